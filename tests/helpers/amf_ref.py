"""Torch-CPU restatement of AMF_model (elliot/recommender/adversarial/AMF/AMF_model.py) for the AMF tests.

Written as the LOSS, gradients from autograd: it shares no hand-derived formula with el_amf.hip.  Every function runs in the dtype
of the tensors it is given (float64 = the reference value, float32 = the yardstick of the tolerance).

  call(adversarial=False) gathers from Gu + dGu, Gi + dGi; call(adversarial=True) from the plain tables (:58-63) -- as written.
  train_step (:70-105), build_perturbation (:133-161), build_msap_perturbation (:163-197), predict (:108-113).
The optimiser is oracle/bprmf_batch.adam_tf_sparse_apply (Keras' sparse apply: every row of m, v, theta moves).

make_case() hands out the edge shapes of tests/test_gpu_amf.py and asserts, on the CPU, that no x or x~ lies within 1e-3 of the
clip bound (planted clipped triplets sit at <= -81) and that every row norm |g| is exactly 0 or >= 1e-3: neither the clip nor the
1e-12 floor of l2_normalize is decided by rounding.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import bprmf_batch

PAD = 3                      # foreign rows in front of every device table of the edge tests
U, I = 37, 23


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def _idx(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int64)


def scores(Gu, Gi, Bi, u, i, j):
    """x = x_ui - x_uj of call() (:65) on the given tables."""
    gu, gi, gj = Gu[u], Gi[i], Gi[j]
    bi, bj = Bi[i], Bi[j]
    return (bi + (gu * gi).sum(1)) - (bj + (gu * gj).sum(1)), (gu, gi, gj, bi, bj)


def bpr_term(x):
    return torch.logaddexp(torch.zeros_like(x), -torch.clamp(x, -80.0, 1e8)).sum()


def reg_term(rows, l_w, l_b):
    gu, gi, gj, bi, bj = rows
    l2 = lambda t: (t * t).sum() / 2
    return l_w * (l2(gu) + l2(gi) + l2(gj)) + l_b * l2(bi) + l_b * l2(bj) / 10


def normalize(g):
    """tf.nn.l2_normalize(g, 1)."""
    return g * torch.rsqrt(torch.clamp((g * g).sum(1, keepdim=True), min=1e-12))


class Model:
    """Variables of AMF_model in `dtype` (torch CPU)."""

    def __init__(self, Gu, Gi, Bi, l_w, l_b, eps, l_adv, dtype=torch.float64, dGu=None, dGi=None):
        self.dtype = dtype
        self.Gu, self.Gi, self.Bi = _t(Gu, dtype).clone(), _t(Gi, dtype).clone(), _t(Bi, dtype).clone()
        self.dGu = torch.zeros_like(self.Gu) if dGu is None else _t(dGu, dtype).clone()
        self.dGi = torch.zeros_like(self.Gi) if dGi is None else _t(dGi, dtype).clone()
        self.l_w, self.l_b, self.eps, self.l_adv = l_w, l_b, eps, l_adv
        self.m = [torch.zeros_like(t) for t in (self.Bi, self.Gu, self.Gi)]
        self.v = [torch.zeros_like(t) for t in (self.Bi, self.Gu, self.Gi)]
        self.step = 0
        self.xs = []                                          # every x / x~ evaluated (make_case checks the clip distance)
        self.norms = []                                       # every row norm l2_normalize saw

    def _loss(self, Gu, Gi, Bi, batch, perturbed):
        u, i, j = (_idx(b) for b in batch)
        x, rows = scores(Gu + self.dGu if perturbed else Gu, Gi + self.dGi if perturbed else Gi, Bi, u, i, j)
        self.xs.append(x.detach().to(torch.float64).numpy())
        return x, rows

    def _perturbation_gradient(self, batch, perturbed):
        """grad of [sum l(x) + reg] w.r.t. (Gu, Gi), delta a constant (tape_adv, :141-158 / :173-190)."""
        Gu, Gi = self.Gu.clone().requires_grad_(True), self.Gi.clone().requires_grad_(True)
        x, rows = self._loss(Gu, Gi, self.Bi, batch, perturbed)
        gu, gi = torch.autograd.grad(bpr_term(x) + reg_term(rows, self.l_w, self.l_b), [Gu, Gi])
        for g in (gu, gi):
            self.norms.append(torch.sqrt((g * g).sum(1)).to(torch.float64).numpy())
        return gu, gi

    def build_perturbation(self, batch):
        self.dGu, self.dGi = torch.zeros_like(self.dGu), torch.zeros_like(self.dGi)
        gu, gi = self._perturbation_gradient(batch, perturbed=True)          # (delta is zero: the plain rows)
        self.dGu, self.dGi = normalize(gu) * self.eps, normalize(gi) * self.eps

    def build_msap_perturbation(self, batch, eps_iter, nb_iter):
        self.dGu, self.dGi = torch.zeros_like(self.dGu), torch.zeros_like(self.dGi)
        for _ in range(nb_iter):
            gu, gi = self._perturbation_gradient(batch, perturbed=True)
            self.dGu = torch.clamp(self.dGu + normalize(gu) * eps_iter, -self.eps, self.eps)
            self.dGi = torch.clamp(self.dGi + normalize(gi) * eps_iter, -self.eps, self.eps)

    def gradients(self, batch, adversarial):
        """(loss, dBi, dGu, dGi) of train_step (:72-102); adversarial=True also rebuilds delta (:91)."""
        Bi, Gu, Gi = (t.clone().requires_grad_(True) for t in (self.Bi, self.Gu, self.Gi))
        x, rows = self._loss(Gu, Gi, Bi, batch, perturbed=True)
        loss = bpr_term(x) + reg_term(rows, self.l_w, self.l_b)
        if adversarial:
            self.build_perturbation(batch)
            xa, _ = self._loss(Gu, Gi, Bi, batch, perturbed=False)
            loss = loss + self.l_adv * bpr_term(xa)
        g = torch.autograd.grad(loss, [Bi, Gu, Gi])
        return (loss.detach(),) + tuple(g)

    def train_step(self, batch, adversarial, lr):
        loss, *g = self.gradients(batch, adversarial)
        self.step += 1
        for th, m, v, gg in zip((self.Bi, self.Gu, self.Gi), self.m, self.v, g):
            bprmf_batch.adam_tf_sparse_apply(th.numpy(), m.numpy(), v.numpy(), gg.numpy(), lr, self.step)      # in place
        return loss

    def predict(self, start, stop, adversarial):
        if adversarial:
            return self.Bi + (self.Gu[start:stop] + self.dGu[start:stop]) @ (self.Gi + self.dGi).T
        return self.Bi + self.Gu[start:stop] @ self.Gi.T


def bound(ref64, ref32):
    """Tolerance of one compared array: 4 x the distance between the restatement's own float32 and float64 runs, floored at one
    float32 ulp of the array's largest magnitude."""
    a, b = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    big = float(np.max(np.abs(a))) if a.size else 0.0
    return max(4.0 * float(np.max(np.abs(a - b))) if a.size else 0.0, float(np.spacing(np.float32(big))))


def distance(got, ref64):
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)))) if np.asarray(got).size else 0.0


def make_case(F, B, seed=0, second=False):
    """Tables and one batch of the edge shape: U = 37, I = 23; one user in half of the triplets, item 1 positive in some triplets and
    negative in others, item 2 only ever negative, items 3 and 4 with identical rows met by one triplet (l_w = 0: that user's
    gradient row is exactly 0), triplets clipped at <= -81.  second=True: another batch over the same tables that shares some rows
    with the first and leaves others (users >= 30, items >= 18) alone."""
    rs = np.random.RandomState(1000 * F + B + seed)
    Gu = rs.uniform(-0.5, 0.5, (U, F)).astype(np.float32)
    Gi = rs.uniform(-0.5, 0.5, (I, F)).astype(np.float32)
    Bi = rs.uniform(-0.2, 0.2, I).astype(np.float32)
    Gi[4] = Gi[3]
    Bi[4] = Bi[3]
    Bi[5], Bi[6] = -45.0, 45.0                                # (5, 6) as (pos, neg): x ~ -90, clipped, no gradient
    hi_u, hi_i = (30, 18) if second else (U, I)
    lo_u = 8 if second else 0
    u = rs.randint(lo_u, hi_u, B)
    i = rs.randint(7, hi_i, B)
    j = rs.randint(7, hi_i, B)
    j = np.where(j == i, 7 + (j - 7 + 1) % (hi_i - 7), j)
    u[::2] = 9                                                # the long user segment
    u[u == 7] = 8
    if B >= 16:                                               # more occurrences of the mixed, the negative-only and the clipped rows
        u[1], i[1], j[1] = 15, 1, 2
        u[3], i[3], j[3] = 16, 11, 1
        u[5], i[5], j[5] = 9, 5, 6
    plant = [(11, 1, 8), (12, 9, 1), (13, 10, 2), (14, 5, 6), (7, 3, 4)]   # user 7 meets only the twin items
    for k, (pu, pi, pj) in enumerate(plant[:B]):
        u[B - 1 - k], i[B - 1 - k], j[B - 1 - k] = pu, pi, pj
    return SimpleNamespace(Gu=Gu, Gi=Gi, Bi=Bi, batch=(u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)), F=F, B=B,
                           l_w=0.0, l_b=0.05, eps=0.5, l_adv=0.7, lr=0.005)


class CaseRejected(Exception):
    """A generated case breaks the helper's promise: the caller draws another one (never a wider tolerance)."""


def check_case(models):
    """The helper's promise about every case it hands out (module docstring), over everything `models` evaluated."""
    for m in models:
        for x in m.xs:
            if not ((np.abs(x + 80.0) > 1e-3).all() and ((x > -80.0) | (x <= -81.0)).all()):
                raise CaseRejected("a score difference within 1e-3 of the clip bound, or a clipped triplet above -81")
        for n in m.norms:
            if not ((n == 0.0) | (n >= 1e-3)).all():
                raise CaseRejected("a row norm between 0 and 1e-3")
