"""Torch-CPU restatement of VBPRModel (elliot/recommender/visual_recommenders/VBPR/VBPR_model.py) for the VBPR tests.

Written as the LOSS on the gathered [B, D] feature blocks, exactly as the file forms it, gradients from autograd: it shares no
hand-derived formula (and no distinct-item algebra) with el_vbpr.hip.  Every function runs in the dtype of the model (float64 =
the reference value, float32 = the yardstick of the tolerance, tests/helpers/amf_ref.bound).

  call (:56-67), train_step (:70-95: loss, six gradients, one Adam move), predict_item_batch (:104-108).
  `predict` (:98-101) reads self.F, which nothing sets: it cannot run and is not restated.
The optimiser: Bi, Gu, Gi, Tu are gathered, their gradients are IndexedSlices -> oracle/bprmf_batch.adam_tf_sparse_apply (every row
moves); E and Bp get dense gradients -> TensorFlow's fused ApplyAdam as oracle/multi_vae.py steps its weights (delta form).

`variant` builds the function's NEIGHBOURS, which the fixture test must tell from it: "neg_bias_full" drops the / 10 on the
negative item's bias term, "l_e_per_sample" multiplies the E / Bp regulariser by the batch size, "no_l_w_on_Tu" leaves theta_u
out of the l_w term.

make_case() hands out the edge batches of tests/test_gpu_vbpr.py on U = 7, I = 65 and check_case() asserts, on the CPU, that no
x lies within 1e-3 of the clip bound (planted clipped triplets sit at <= -81): the clip is never decided by rounding.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import bprmf_batch, tf_clauses
from tests.helpers.amf_ref import CaseRejected, bound, distance  # noqa: F401  (re-exported: the tests' tolerance)

U, I = 7, 65
NAMES = ("Bi", "Gu", "Gi", "Tu", "E", "Bp")            # the order of train_step's gradient list (:92-93)


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def _idx(x):
    return torch.as_tensor(np.asarray(x).reshape(-1), dtype=torch.int64)


def adam_dense_apply(theta, m, v, g, lr, t):
    """TensorFlow's fused ApplyAdam (dense gradients), in place -- oracle/multi_vae.py's step."""
    f = np.float32
    if not tf_clauses.get("adam_dense_uses_delta_form"):
        return bprmf_batch.adam_tf_sparse_apply(theta, m, v, g, lr, t)
    a = bprmf_batch.adam_lr_t(lr, t)
    m += (g - m) * tf_clauses.one_minus(bprmf_batch.BETA1)
    v += (g * g - v) * tf_clauses.one_minus(bprmf_batch.BETA2)
    theta -= (m * a) / (np.sqrt(v) + f(bprmf_batch.EPS))


class Model:
    """Variables of VBPRModel in `dtype` (torch CPU).  feat: the [I, D] feature matrix; a batch's feature blocks are feat[pos], feat[neg]."""

    def __init__(self, Gu, Gi, Bi, Tu, E, Bp, feat, l_w, l_b, l_e, dtype=torch.float64, variant=None):
        self.dtype, self.variant = dtype, variant
        self.Bi, self.Gu, self.Gi = _t(Bi, dtype).clone(), _t(Gu, dtype).clone(), _t(Gi, dtype).clone()
        self.Tu, self.E = _t(Tu, dtype).clone(), _t(E, dtype).clone()
        self.Bp = _t(Bp, dtype).clone().reshape(-1, 1)
        self.feat = _t(feat, dtype)
        self.l_w, self.l_b, self.l_e = l_w, l_b, l_e
        self.m = {n: torch.zeros_like(getattr(self, n)) for n in NAMES}
        self.v = {n: torch.zeros_like(getattr(self, n)) for n in NAMES}
        self.step = 0
        self.xs = []                                          # every x evaluated (check_case reads the clip distance)

    @staticmethod
    def call(V, user, item, feature_i):
        """call (:56-67) on the variables V = (Bi, Gu, Gi, Tu, E, Bp)."""
        Bi, Gu, Gi, Tu, E, Bp = V
        beta_i, gamma_u, theta_u, gamma_i = Bi[item], Gu[user], Tu[user], Gi[item]
        xui = beta_i + (gamma_u * gamma_i).sum(1) + (theta_u * (feature_i @ E)).sum(1) + (feature_i @ Bp).squeeze(1)
        return xui, gamma_u, gamma_i, feature_i, theta_u, beta_i

    def loss(self, V, batch):
        """The loss of train_step (:73-90)."""
        user, pos, neg = (_idx(b) for b in batch)
        Bi, Gu, Gi, Tu, E, Bp = V
        xu_pos, gamma_u, gamma_pos, _, theta_u, beta_pos = self.call(V, user, pos, self.feat[pos])
        xu_neg, _, gamma_neg, _, _, beta_neg = self.call(V, user, neg, self.feat[neg])
        x = xu_pos - xu_neg
        self.xs.append(x.detach().to(torch.float64).numpy())
        loss = torch.logaddexp(torch.zeros_like(x), -torch.clamp(x, -80.0, 1e8)).sum()
        l2 = lambda t: (t * t).sum() / 2                      # noqa: E731  (tf.nn.l2_loss)
        rows = [l2(gamma_u), l2(gamma_pos), l2(gamma_neg)] + ([] if self.variant == "no_l_w_on_Tu" else [l2(theta_u)])
        neg_bias = self.l_b * l2(beta_neg) / (1 if self.variant == "neg_bias_full" else 10)
        dense = self.l_e * (l2(E) + l2(Bp)) * (len(user) if self.variant == "l_e_per_sample" else 1)
        return loss + self.l_w * sum(rows) + self.l_b * l2(beta_pos) + neg_bias + dense

    def variables(self):
        return tuple(getattr(self, n) for n in NAMES)

    def gradients(self, batch):
        """(loss, dBi, dGu, dGi, dTu, dE, dBp), the IndexedSlices summed into dense arrays (tape.gradient, :92)."""
        V = tuple(t.clone().requires_grad_(True) for t in self.variables())
        loss = self.loss(V, batch)
        g = torch.autograd.grad(loss, V)
        return (loss.detach(),) + tuple(g)

    def train_step(self, batch, lr):
        loss, *g = self.gradients(batch)
        self.step += 1
        for n, gg in zip(NAMES, g):
            apply = adam_dense_apply if n in ("E", "Bp") else bprmf_batch.adam_tf_sparse_apply
            apply(getattr(self, n).numpy(), self.m[n].numpy(), self.v[n].numpy(), gg.numpy(), lr, self.step)      # in place
        return loss

    def predict_item_batch(self, start, stop, start_item, stop_item, feat):
        """:104-108; `feat` holds the rows of items start_item .. stop_item (inclusive, as the file slices)."""
        sl = slice(start_item, stop_item + 1)
        feat = _t(feat, self.dtype)
        return self.Bi[sl] + self.Gu[start:stop] @ self.Gi[sl].T + self.Tu[start:stop] @ (feat @ self.E).T + (feat @ self.Bp).squeeze(1)

    def predict_all(self):
        return self.predict_item_batch(0, self.Gu.shape[0], 0, self.Gi.shape[0] - 1, self.feat)


KINDS = ("mixed", "one_user", "one_pair", "long_item", "all_items")


def make_case(F, Fd, D, B, kind="mixed", seed=0, l_w=0.05, l_e=0.01):
    """Variables, features and one batch on U = 7, I = 65.
      mixed      random triplets; from B >= 16: item 1 positive in some triplets and negative in others, item 2 only ever negative, the
                 triplet (5, 6) with Bi = -/+ 45 sits at x ~ -90 (clipped, no gradient); B = 2 holds the clipped triplet too
      one_user   every triplet belongs to user 3
      one_pair   every triplet is (., 8, 9)
      long_item  item 10 is the positive of 5 triplets in 6 and the negative of every 97th: its segment is longer than any lane group's
                 chunk x lanes (needs B > 1024)
      all_items  the positives run through every item in turn (needs B >= 65)"""
    assert kind in KINDS
    rs = np.random.RandomState(100000 * F + 1000 * Fd + 7 * D + B + 31 * KINDS.index(kind) + seed)
    Gu = rs.uniform(-0.5, 0.5, (U, F)).astype(np.float32)
    Gi = rs.uniform(-0.5, 0.5, (I, F)).astype(np.float32)
    Bi = rs.uniform(-0.2, 0.2, I).astype(np.float32)
    Tu = rs.uniform(-0.5, 0.5, (U, Fd)).astype(np.float32)
    E = rs.uniform(-0.5, 0.5, (D, Fd)).astype(np.float32)
    Bp = rs.uniform(-0.5, 0.5, (D, 1)).astype(np.float32)
    feat = (rs.uniform(0.0, 2.0, (I, D)) / np.sqrt(D)).astype(np.float32)          # non-negative, as CNN features after a ReLU
    Bi[5], Bi[6] = -45.0, 45.0
    u = rs.randint(0, U, B)
    i = rs.randint(7, I, B)
    j = rs.randint(7, I, B)
    j = np.where(j == i, 7 + (j - 7 + 1) % (I - 7), j)
    if kind == "one_user":
        u[:] = 3
    elif kind == "one_pair":
        i[:], j[:] = 8, 9
    elif kind == "long_item":
        assert B > 1024
        i[np.arange(B) % 6 != 0] = 10
        j[i == 10] = np.where(j[i == 10] == 10, 11, j[i == 10])
        sel = (np.arange(B) % 97 == 0) & (i != 10)
        j[sel] = 10
    elif kind == "all_items":
        assert B >= I
        i = np.arange(B) % I
        j = (i + 1 + rs.randint(0, I - 1, B)) % I
    if kind in ("mixed", "one_user") and B >= 16:
        i[1], j[1] = 1, 2
        i[3], j[3] = 11, 1
        i[5], j[5] = 5, 6
        i[7], j[7] = 12, 2
    elif kind == "mixed" and B == 2:
        i[1], j[1] = 5, 6
    return SimpleNamespace(Gu=Gu, Gi=Gi, Bi=Bi, Tu=Tu, E=E, Bp=Bp, feat=feat, F=F, Fd=Fd, D=D, B=B, kind=kind,
                           batch=(u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)), l_w=l_w, l_b=0.05, l_e=l_e, lr=0.005)


def model_of(case, dtype, variant=None):
    return Model(case.Gu, case.Gi, case.Bi, case.Tu, case.E, case.Bp, case.feat, case.l_w, case.l_b, case.l_e, dtype, variant)


def check_case(models):
    """The helper's promise about every case it hands out (module docstring), over everything `models` evaluated."""
    for m in models:
        for x in m.xs:
            if not ((np.abs(x + 80.0) > 1e-3).all() and ((x > -80.0) | (x <= -81.0)).all()):
                raise CaseRejected("a score difference within 1e-3 of the clip bound, or a clipped triplet above -81")
