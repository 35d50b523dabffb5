"""Torch-CPU restatement of FactorizationMachineModel (elliot/recommender/latent_factor_models/FM/factorization_machine_model.py)
for the FM tests, in the dtype of the model (float64 = the reference value, float32 = the yardstick of amf_ref.bound).

Written on DENSE one-hot rows X [B, U + I + nF] as the reference is fed them (prepare_fm_transaction), with its own expression
1/2 (sum(M M^T) - sum(M^2)) over the masked rows M -- the pairwise products, not the squared sum -- and gradients from autograd: it
shares no factoring through the item with el_fm.hip.  `factored()` is the form the kernels use (s_i, q_i, l_i); the host test pins
it to the one-hot form.  The optimiser is TensorFlow's fused dense ApplyAdam (vbpr_ref.adam_dense_apply) on E, w and g0.

make_case(): U = 7, I = 65 (I = 300 for kind "every": above the long-list threshold of k_fm_feat, 256).  With nF = 70: item 0 has
no feature, item 1 one, item 2 forty, items 3 and 4 the same three; feature 68 sits on the last item only, which no batch samples;
kind "every" puts feature 67 on every item.  nF = 1: the one feature on every other item.  Batches: sample 1 repeats sample 0,
user 2 is in every other sample, items 0 .. 4 are sampled; kind "long_item" gives item 10 about a fifth of the samples; kind
"second" stays on users < 3 and items 20 .. 29.  Labels are drawn from {0, .., 5}.
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers.amf_ref import bound, distance  # noqa: F401  (re-exported: the tests' tolerance)
from tests.helpers.vbpr_ref import adam_dense_apply

U = 7
NAMES = ("E", "w", "g0")


def attribute_sets(I, nF, rs, every=False):
    if nF == 0:
        return [[] for _ in range(I)]
    if nF == 1:
        return [[0] if i % 2 else [] for i in range(I)]
    sets = [sorted(rs.choice(nF - 3, rs.randint(0, 5), replace=False).tolist()) for _ in range(I)]
    sets[0], sets[1], sets[2], sets[3], sets[4] = [], [3], list(range(40)), [5, 6, 7], [5, 6, 7]
    sets[I - 1] = sorted(set(sets[I - 1]) | {nF - 2})
    return [sorted(set(s) | {nF - 3}) for s in sets] if every else sets


def make_batch(I, B, rs, kind="mixed"):
    if kind == "second":
        u, i = rs.randint(0, 3, B), rs.randint(20, 30, B)
    else:
        u, i = rs.randint(0, U, B), rs.randint(0, I - 1, B)          # (the last item is never sampled)
        u[::2] = 2
        if kind == "long_item":
            i[rs.rand(B) < 0.2] = 10
        for k in range(min(5, max(B - 2, 0))):
            i[2 + k] = k
        if B >= 2:
            u[1], i[1] = u[0], i[0]
    return u.astype(np.int32), i.astype(np.int32), rs.randint(0, 6, B).astype(np.float32)


def make_case(F, B, nF=70, kind="mixed", seed=0):
    I = 300 if kind == "every" else 65
    rs = np.random.RandomState(1000 * F + B + 7 * nF + seed)
    N = U + I + nF
    E = rs.uniform(-0.5, 0.5, (N, F)).astype(np.float32)
    w = rs.uniform(-0.2, 0.2, N).astype(np.float32)
    feats = attribute_sets(I, nF, rs, every=kind == "every")
    return SimpleNamespace(U=U, I=I, nF=nF, F=F, B=B, E=E, w=w, g0=np.float32(0.3), feats=feats, batch=make_batch(I, B, rs, kind),
                           second=make_batch(I, B, rs, "second"), lr=0.005)


def one_hot(case, u, i):
    """prepare_fm_transaction / get_item_fragment: the ones are WRITTEN (a repeated feature counts once)."""
    X = np.zeros((len(u), case.U + case.I + case.nF), np.float64)
    for b, (uu, ii) in enumerate(zip(u, i)):
        X[b, uu] = X[b, case.U + ii] = 1.0
        X[b, [case.U + case.I + f for f in case.feats[ii]]] = 1.0
    return X


class Model:
    def __init__(self, case, dtype=torch.float64):
        self.case, self.dtype = case, dtype
        t = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype).clone()                  # noqa: E731
        self.E, self.w, self.g0 = t(case.E), t(case.w), t(case.g0).reshape(1)
        self.m = {n: torch.zeros_like(getattr(self, n)) for n in NAMES}
        self.v = {n: torch.zeros_like(getattr(self, n)) for n in NAMES}
        self.step = 0

    def call(self, V, X):
        """FactorizationMachineLayer.call on one-hot rows: Linear (:130) + Embedding (:178-180)."""
        E, w, g0 = V
        X = torch.as_tensor(X, dtype=self.dtype)
        pair = ((X @ (E @ E.T)) * X).sum(1)                     # sum(M M^T) of the masked rows
        return g0 + X @ w + 0.5 * (pair - X @ (E * E).sum(1))

    def predict(self, u, i):
        return self.call((self.E, self.w, self.g0), one_hot(self.case, u, i))

    def predict_all(self):
        uu, ii = np.meshgrid(np.arange(self.case.U), np.arange(self.case.I), indexing="ij")
        return self.predict(uu.reshape(-1), ii.reshape(-1)).reshape(self.case.U, self.case.I)

    def factored(self, u, i):
        """g0 + w_u + l_i + e_u . s_i + 1/2 (|s_i|^2 - q_i): the form of el_fm.hip."""
        c, out = self.case, []
        for uu, ii in zip(u, i):
            rows = [c.U + ii] + [c.U + c.I + f for f in c.feats[ii]]
            s, q, l = self.E[rows].sum(0), (self.E[rows] ** 2).sum(), self.w[rows].sum()
            out.append(self.g0[0] + self.w[uu] + l + self.E[uu] @ s + 0.5 * (s @ s - q))
        return torch.stack(out)

    def gradients(self, batch):
        """(loss, dE, dw, dg0) of the Keras MeanSquaredError (:62-69)."""
        u, i, y = batch
        V = tuple(getattr(self, n).clone().requires_grad_(True) for n in NAMES)
        loss = ((torch.as_tensor(y, dtype=self.dtype) - self.call(V, one_hot(self.case, u, i))) ** 2).mean()
        return (loss.detach(),) + torch.autograd.grad(loss, V)

    def train_step(self, batch, lr):
        loss, *g = self.gradients(batch)
        self.step += 1
        for n, gg in zip(NAMES, g):
            adam_dense_apply(getattr(self, n).numpy(), self.m[n].numpy(), self.v[n].numpy(), gg.numpy(), lr, self.step)      # in place
        return loss
