"""Torch-CPU restatement of ConvNeuralMatrixFactorizationModel (elliot/recommender/neural/ConvNeuMF/
convolutional_neural_matrix_factorization_model.py) for the ConvNeuMF tests, in the dtype of the model (float64 = the reference value,
float32 = the yardstick of amf_ref.bound).

`call`, `train_step` and `get_recs` written as the loss: the explicit [B, 1, F, F] outer product through torch.nn.functional.conv2d
(VALID, stride = kernel), sum over the pixels, two linear Dense layers; gradients from autograd; Keras Adam from oracle/bprmf_batch
(sparse apply on the two tables: every row moves) and TF's dense ApplyAdam on the rest.  It shares no factoring through the item, no
patch GEMM and no hand-derived gradient with el_cnmf.hip.

make_case(): U = 70, I = 45.  Embeddings are integers times 2^-ebits, conv kernels and biases integers times 2^-wbits, so every
pre-activation that feeds a ReLU is the same number in float32 and float64 in any order (check_exact asserts it); the Dense weights are
ordinary floats scaled so that x_ui - x_uj spreads over both signs, and no difference lies within 1e-3 of the clip at -80 (asserted in
gradients()).  Batch: user 3 in every other sample, item 5 positive in triplet 1 and negative in triplet 2; the second batch draws its
users from 35 on, so rows of P met by the first batch are not met again.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as fn

from oracle import bprmf_batch
from tests.helpers.amf_ref import bound, distance  # noqa: F401  (re-exported: the tests' tolerance)

U, I = 70, 45


def make_batch(B, rs, second=False):
    u, i, j = rs.randint(35 if second else 0, 35 if not second else U, B), rs.randint(0, I, B), rs.randint(0, I, B)
    if not second:
        u[::2] = 3
        if B >= 3:
            i[1], j[2] = 5, 5
    j = np.where(j == i, (j + 1) % I, j)
    return u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)


def make_case(F, channels, kernels, B, seed=0, ebits=2, wbits=3, l_w=0.005):
    rs = np.random.RandomState(1000 * F + 10 * sum(channels) + B + seed)
    grid = lambda shape, bits: (rs.randint(-4, 5, shape) / 2.0 ** bits).astype(np.float32)      # noqa: E731
    w = {"P": grid((U, F), ebits), "Q": grid((I, F), ebits),
         "conv": [(grid((k, k, a, b), wbits), grid(b, wbits)) for k, a, b in zip(kernels, channels[:-1], channels[1:])]}
    C = channels[-1]
    w["dense"] = [(rs.uniform(-1, 1, (C, C)).astype(np.float32) / C, rs.uniform(-0.1, 0.1, C).astype(np.float32)),
                  (rs.uniform(-1, 1, (C, 1)).astype(np.float32), rs.uniform(-0.1, 0.1, 1).astype(np.float32))]
    case = SimpleNamespace(U=U, I=I, F=F, B=B, channels=list(channels), kernels=list(kernels), weights=w, l_w=l_w, lr=0.005,
                           batch=make_batch(B, rs), second=make_batch(B, rs, second=True))
    x = Model(case).get_recs(0, U).numpy()                                    # spread the scores: standard deviation 2
    w["dense"][1] = (w["dense"][1][0] * np.float32(2.0 / max(x.std(), 1e-30)), w["dense"][1][1])
    return case


def names(case):
    return ["P", "Q"] + [f"{n}{l}" for l in range(len(case.kernels)) for n in "Wb"] + [f"D{q}" for q in range(4)]


class Model:
    def __init__(self, case, dtype=torch.float64):
        w = case.weights
        flat = [w["P"], w["Q"]] + [x for Wb in w["conv"] for x in Wb] + [x for Wb in w["dense"] for x in Wb]
        self.case, self.dtype, self.nl = case, dtype, len(case.kernels)
        self.V = [torch.as_tensor(np.asarray(x)).to(dtype).clone() for x in flat]
        self.m, self.v, self.step = [np.zeros_like(x.numpy()) for x in self.V], [np.zeros_like(x.numpy()) for x in self.V], 0

    def call(self, V, user, item, masks=None):
        """(prediction, gamma_u, gamma_i, the pre-activations of the conv layers); masks = the two Dropout layers' factors [B, C]."""
        p, q = V[0][user], V[1][item]
        x, pre = (p.unsqueeze(2) * q.unsqueeze(1)).unsqueeze(1), []
        for l, k in enumerate(self.case.kernels):
            pre.append(fn.conv2d(x, V[2 + 2 * l].permute(3, 2, 0, 1), V[3 + 2 * l], stride=k))
            x = torch.relu(pre[-1])
        z, (Wd1, bd1, Wd2, bd2) = x.sum((2, 3)), V[2 + 2 * self.nl:]
        h = (z * masks[0] if masks is not None else z) @ Wd1 + bd1
        return ((h * masks[1] if masks is not None else h) @ Wd2.reshape(-1, 1)).reshape(-1) + bd2, p, q, pre

    def gradients(self, batch, masks=None):
        """(loss, x_ui - x_uj, the gradients in names() order) of train_step; masks [2, 2, B, C] (call, layer, sample, unit)."""
        u, i, j = (torch.as_tensor(np.asarray(x)).long() for x in batch)
        V = [x.clone().requires_grad_(True) for x in self.V]
        mk = [None, None] if masks is None else [[torch.as_tensor(np.asarray(m)).to(self.dtype) for m in masks[c]] for c in (0, 1)]
        xp, gu, gi, _ = self.call(V, u, i, mk[0])
        xn, gu, gj, _ = self.call(V, u, j, mk[1])
        d = xp - xn
        assert (np.abs(d.detach().numpy() + 80.0) > 1e-3).all(), "a score difference within 1e-3 of the clip"
        l2 = lambda t: (t * t).sum() / 2                                                             # noqa: E731
        loss = fn.softplus(-torch.clamp(d, -80.0, 1e8)).sum() + self.case.l_w * (l2(gu) + l2(gi) + l2(gj))
        return (loss.detach().double(), d.detach()) + tuple(torch.autograd.grad(loss, V))

    def train_step(self, batch, masks=None):
        loss, _, *g = self.gradients(batch, masks)
        self.step += 1
        f = self.V[0].numpy().dtype.type
        lr_t = f(bprmf_batch.adam_lr_t(self.case.lr, self.step))
        for k, (th, m, v, gg) in enumerate(zip(self.V, self.m, self.v, g)):
            gg = gg.numpy()
            if k < 2:                                                        # Keras' sparse apply on a table: every row moves
                bprmf_batch.adam_tf_sparse_apply(th.numpy(), m, v, gg, self.case.lr, self.step)
            else:                                                            # TF dense ApplyAdam
                m += (gg - m) * f(1 - np.float32(0.9))
                v += (gg * gg - v) * f(1 - np.float32(0.999))
                th.numpy()[...] -= (m * lr_t) / (np.sqrt(v) + f(1e-7))
        return loss

    def get_recs(self, start, stop):
        """get_recs for the users [start, stop) against all items: [Uc, I]."""
        n, c = stop - start, self.case
        user = torch.arange(start, stop).repeat_interleave(c.I)
        with torch.no_grad():
            return self.call(self.V, user, torch.arange(c.I).repeat(n))[0].reshape(n, c.I)


def check_exact(case, batch):
    """What the bounds rest on: every conv pre-activation of both calls is the same number in float32 and float64."""
    u, i, j = (torch.as_tensor(np.asarray(x)).long() for x in batch)
    m64, m32 = Model(case), Model(case, torch.float32)
    with torch.no_grad():
        for item in (i, j):
            for a, b in zip(m64.call(m64.V, u, item)[3], m32.call(m32.V, u, item)[3]):
                assert torch.equal(a, b.double()), "a float32 pre-activation differs from the float64 one"
