"""Torch-CPU restatement of FISM_model (elliot/recommender/latent_factor_models/FISM/FISM_model.py) for the FISM tests, in the dtype
of the model (float64 = the reference value, float32 = the yardstick of amf_ref.bound).

A literal transcription of `call` (:61-76), `train_step` (:78-92) and `batch_predict` (:119-144): the padded history matrix and its
mask (create_history_item_matrix, pads = item id 0), [B, L, F] gathers, the loss called as loss(output, label) -- Keras
BinaryCrossentropy(y_true = output, y_pred = label), in float64 because the labels are --, gradients from autograd.  It holds no
hand-derived gradient and shares no factoring through the batch's distinct users with el_fism.hip.  loss="bce" is the cross-entropy
that was meant; pad=False masks the padded slots out of the regulariser and out of batch_predict.  The loss is a sum over samples,
so gradients() walks the batch in chunks and adds (the [B, L, F] block of B = 4097 does not have to exist at once).  coef =
n_u^-alpha is float32 in both runs, as the reference's float32 history_lens make it.  Keras Adam's every-row sparse apply is
oracle.bprmf_batch.adam_tf_sparse_apply, the one the point-wise restatement steps with.

make_case(): U = I = 600, L = 515.  Users 0 .. 5 have histories of 1, 2, 255, 256, 257, 515 items, the others 1 .. 34 in shuffled
stored order; item 10 is held by 515 users, 11 by 257, 12 by 256 (none of them ever in a batch), 13 by one, 14 by none, item 0 by
users 1 and 6 .. 15.  Batches draw users below 300 only: user 4 is in every other sample, sample 0 targets an item of its own user's
history, item 30 is the target of a fifth of the samples, item 599 of none; labels from {0, 0.5, 1, 3, 5}.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle.bprmf_batch import adam_tf_sparse_apply
from tests.helpers.amf_ref import bound, distance  # noqa: F401  (re-exported: the tests' tolerance)

U = I = 600
NAMES = ("Gi", "Gj", "Bu", "Bi")
PLANTED = (1, 2, 255, 256, 257, 515)
EPS = 1e-7


def make_batch(B, rs, hist, second=False):
    u, i = rs.randint(0, 300, B), rs.randint(0, I - 1, B)
    if not second:
        u[::2] = 4
        i[rs.rand(B) < 0.2] = 30
        k = min(len(PLANTED), B)
        u[:k] = [5, 0, 1, 2, 3, 4][:k]
        i[0] = hist[5][0]
    return u.astype(np.int32), i.astype(np.int32), rs.choice([0.0, 0.5, 1.0, 3.0, 5.0], B).astype(np.float32)


def make_case(F, B, alpha=0.5, seed=0):
    rs = np.random.RandomState(1000 * F + B + seed)
    hist = [rs.choice(np.arange(20, I), n, replace=False) for n in PLANTED]
    hist[1][0] = 0
    for u in range(len(PLANTED), U):
        own = rs.choice(np.arange(20, I), rs.randint(1, 31), replace=False)
        extra = [k for k, users in ((10, range(6, 521)), (11, range(100, 357)), (12, range(340, 596)), (13, (7,)), (0, range(6, 16))) if u in users]
        hist.append(rs.permutation(np.concatenate([own, extra]).astype(np.int64)))
    lens = np.array([len(h) for h in hist])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    coef = np.power(lens.astype(np.float32), np.float32(-alpha)).astype(np.float32)
    t = lambda lo, hi, *s: rs.uniform(lo, hi, s).astype(np.float32)                       # noqa: E731
    return SimpleNamespace(U=U, I=I, F=F, B=B, L=int(lens.max()), alpha=alpha, hist=hist, lens=lens, indptr=indptr,
                           indices=np.concatenate(hist).astype(np.int32), coef=coef, Gi=t(-0.3, 0.3, I, F), Gj=t(-0.3, 0.3, I, F),
                           Bu=t(-0.2, 0.2, U), Bi=t(-0.2, 0.2, I), beta=0.01, lam=0.02, gamma=0.03, lr=0.005,
                           batch=make_batch(B, rs, hist), second=make_batch(B, rs, hist, second=True))


def l2_loss(x):
    return (x * x).sum() / 2


class Model:
    def __init__(self, case, dtype=torch.float64, pad=True, loss="reference"):
        self.case, self.dtype, self.pad, self.loss_kind = case, dtype, pad, loss
        self.hist = torch.zeros((case.U, case.L), dtype=torch.int64)                      # create_history_item_matrix (:146-168)
        self.mask = torch.zeros((case.U, case.L), dtype=dtype)
        for u, h in enumerate(case.hist):
            self.hist[u, :len(h)] = torch.as_tensor(h)
            self.mask[u, :len(h)] = 1
        self.coef = torch.as_tensor(case.coef).to(dtype)                                  # tf.pow(item_num, -alpha) in float32
        for n in NAMES:
            setattr(self, n, torch.as_tensor(getattr(case, n)).to(dtype).clone())
        self.m = {n: np.zeros_like(getattr(self, n).numpy()) for n in NAMES}
        self.v = {n: np.zeros_like(getattr(self, n).numpy()) for n in NAMES}
        self.step = 0

    def call(self, V, user, item):
        Gi, Gj, Bu, Bi = V
        batch_mask_mat = self.mask[user]
        user_history = Gi[self.hist[user]]                                                # batch_size x max_len x embedding_size
        target, user_bias, item_bias = Gj[item], Bu[user], Bi[item]
        similarity = torch.matmul(user_history, target.unsqueeze(2)).squeeze(2)
        similarity = batch_mask_mat * similarity
        scores = 1 / (1 + torch.exp(-(self.coef[user] * similarity.sum(1) + user_bias + item_bias)))
        return scores, user_bias, item_bias, user_history, target, batch_mask_mat

    def chunk_loss(self, V, user, item, label, B):
        """train_step's loss (:83-87) over some samples of a batch of B: the mean's share plus the regulariser's."""
        c = self.case
        output, user_bias, item_bias, source, target, mask = self.call(V, user, item)
        if not self.pad:
            source = source * mask.unsqueeze(2)
        reg = c.lam * l2_loss(user_bias) + c.gamma * l2_loss(item_bias) + c.beta * (l2_loss(source) + l2_loss(target))
        label = torch.as_tensor(label, dtype=torch.float64)
        if self.loss_kind == "reference":                                                 # BinaryCrossentropy()(y_true = output, y_pred = label)
            y_true, y_pred = output.double(), torch.clamp(label, EPS, 1 - EPS)
        else:
            y_true, y_pred = (label > 0).to(self.dtype), torch.clamp(output, EPS, 1 - EPS)
        bce = y_true * torch.log(y_pred + EPS) + (1 - y_true) * torch.log(1 - y_pred + EPS)
        return (-bce).sum().double() / B + reg.double()

    def gradients(self, batch, chunk=256):
        """(loss, dGi, dGj, dBu, dBi) of train_step (:80-89)."""
        u, i, y = (np.asarray(x) for x in batch)
        V = tuple(getattr(self, n).clone().requires_grad_(True) for n in NAMES)
        loss, grads = torch.zeros((), dtype=torch.float64), [torch.zeros_like(v) for v in V]
        for s in range(0, len(u), chunk):
            part = self.chunk_loss(V, torch.as_tensor(u[s:s + chunk].astype(np.int64)), torch.as_tensor(i[s:s + chunk].astype(np.int64)),
                                   y[s:s + chunk], len(u))
            for g, d in zip(grads, torch.autograd.grad(part, V)):
                g += d
            loss += part.detach()
        return (loss,) + tuple(grads)

    def train_step(self, batch, lr):
        loss, *g = self.gradients(batch)
        self.step += 1
        for n, gg in zip(NAMES, g):
            adam_tf_sparse_apply(getattr(self, n).numpy(), self.m[n], self.v[n], gg.numpy(), lr, self.step)      # in place
        return loss

    def batch_predict(self, chunk=100):
        """batch_predict (:119-144) for all users: the similarity summed over ALL L slots (pad=False: the mask applied)."""
        out = []
        for s in range(0, self.case.U, chunk):
            user = torch.arange(s, min(s + chunk, self.case.U))
            user_history = self.Gi[self.hist[user]]                                       # bs x inter_num x embedding_size
            similarity = torch.matmul(user_history, self.Gj.T)                            # bs x inter_num x target_items
            if not self.pad:
                similarity = similarity * self.mask[user].unsqueeze(2)
            prod = self.coef[user].unsqueeze(1) * similarity.sum(1)
            out.append(1 / (1 + torch.exp(-(prod + self.Bu[user].unsqueeze(1) + self.Bi))))
        return torch.cat(out)


def factored(case, batch, pad_len, loss="reference"):
    """The gradient formulas of el_fism.hip (include/elliot_hip.h, el_fism_grads), evaluated in numpy float64: per distinct user T_u,
    cnt_u, R_u = coef_u T_u, then the fan-out over the histories.  Returns (dGi, dGj, dBu, dBi)."""
    u, i, y = (np.asarray(x) for x in batch)
    Gi, Gj, Bu, Bi = (np.asarray(getattr(case, n), np.float64) for n in NAMES)
    coef, B = case.coef.astype(np.float64), len(u)
    p = np.stack([Gi[case.hist[uu]].sum(0) for uu in u])
    out = 1 / (1 + np.exp(-(coef[u] * (p * Gj[i]).sum(1) + Bu[u] + Bi[i])))
    if loss == "reference":
        yh = np.clip(y.astype(np.float64), EPS, 1 - EPS)
        d = -(np.log(yh + EPS) - np.log(1 - yh + EPS)) / B
    else:
        pc = np.clip(out, EPS, 1 - EPS)
        d = np.where((out >= EPS) & (out <= 1 - EPS), np.where(y > 0, -1 / (pc + EPS), 1 / (1 - pc + EPS)), 0.0) / B
    c = d * out * (1 - out)
    g = [np.zeros_like(Gi), np.zeros_like(Gj), np.zeros_like(Bu), np.zeros_like(Bi)]
    np.add.at(g[2], u, c + case.lam * Bu[u])
    np.add.at(g[3], i, c + case.gamma * Bi[i])
    np.add.at(g[1], i, c[:, None] * coef[u][:, None] * p + case.beta * Gj[i])
    for uu in np.unique(u):
        sel = u == uu
        R, cnt = coef[uu] * (c[sel, None] * Gj[i[sel]]).sum(0), sel.sum()
        np.add.at(g[0], case.hist[uu], R + case.beta * cnt * Gi[case.hist[uu]])
    if pad_len:
        g[0][0] += case.beta * Gi[0] * (pad_len - case.lens[u]).sum()
    return g
