"""Torch-CPU restatement of DeepMatrixFactorizationModel (elliot/recommender/neural/DMF/deep_matrix_factorization_model.py) for the
DMF tests, in the dtype of the model (float64 = the reference value, float32 = the yardstick of amf_ref.bound).

A literal transcription of `call` (:84-91), `train_step` (:94-105) and `get_recs` (:119-132): the two dense "embeddings" R and R^T,
one dense row per SAMPLE through the MLPs, tf.nn.l2_normalize(., 0) along the batch axis (axis="row": along the feature axis),
Keras BinaryCrossentropy on label / max_rating, gradients from autograd, TF's dense ApplyAdam.  It shares no distinct-row factoring,
no piece cut and no hand-derived gradient with el_dmf.hip.

make_case(): U = I = 300, integer ratings 1 .. 5.  Users 0 .. 8 rate 1, 7, 8, 9, 17, 28, 33, 40, 137 items, items 0 .. 8 are rated by as
many users (one, piece - 1, piece, piece + 1, 3, 4, 5, 5 and 18 pieces at fism_piece = 8); the others rate 1 .. 12 items.  Batches
draw users and items below 150 (the second batch users from 75 on, so that many kernel rows are reached by the first batch alone): behind the nine planted pairs user 4 is in every other sample; the kernel rows of items rated above user 150 only are reached by
no batch row.  Every kernel and bias that feeds a ReLU is an integer times 2^-4, so every such pre-activation is exact in float32 in any
order (check_exact); the last layers are ordinary floats scaled so that the dot product spreads over (-inf, 0), (0, 1) and (1, inf).  last_bias=False (the scoring case) leaves the last biases
zero: get_recs' batch-axis cosine keeps only the SIGN of every q[i, d], and with a common positive bias most items would share one
sign pattern and tie exactly.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle.bprmf_batch import adam_lr_t
from tests.helpers.amf_ref import bound, distance  # noqa: F401  (re-exported: the tests' tolerance)

U = I = 300
PLANTED = (1, 7, 8, 9, 17, 28, 33, 40, 137)
EPS = 1e-7


def make_ratings(rs):
    R = np.zeros((U, I), np.float32)
    for u in range(U):
        n = PLANTED[u] if u < len(PLANTED) else rs.randint(1, 13)
        R[u, rs.choice(np.arange(20, I), n, replace=False)] = rs.randint(1, 6, n)
    for i, n in enumerate(PLANTED):
        R[rs.choice(np.arange(20, U), n, replace=False), i] = rs.randint(1, 6, n)
    return R


def make_batch(B, rs, R, second=False):
    u, i = rs.randint(75 if second else 0, 150, B), rs.randint(0, 150, B)
    if not second:
        k = min(len(PLANTED), B)
        u[:k], i[:k] = np.arange(len(PLANTED))[:k], np.arange(len(PLANTED))[::-1][:k]
        u[k::2] = 4
    y = np.where(rs.rand(B) < 0.5, R[u, i], 0).astype(np.float32)
    return u.astype(np.int32), i.astype(np.int32), np.where(y > 0, y, rs.choice([0.0, 3.0, 5.0], B)).astype(np.float32)


def make_case(user_mlp, item_mlp, B, seed=0, last_bias=True):
    rs = np.random.RandomState(1000 * sum(user_mlp) + 10 * sum(item_mlp) + B + seed)
    R = make_ratings(rs)
    D, w = user_mlp[-1], {}
    for side, first, units in (("user", I, user_mlp), ("item", U, item_mlp)):
        widths, layers = [first] + list(units), []
        for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
            if l < len(units) - 1:
                layers.append((rs.randint(-4, 5, (a, b)).astype(np.float32) / 16, rs.randint(-4, 5, b).astype(np.float32) / 16))
            else:
                layers.append((rs.uniform(-1, 1, (a, b)), np.zeros(b)))
        x = R if side == "user" else R.T                         # scale the linear last layer: entries of rms (0.6 / sqrt D)^(1/2), mean (0.4 / D)^(1/2)
        for W, b in layers[:-1]:
            x = np.maximum(x.astype(np.float64) @ W + b, 0)
        W, b = layers[-1]
        W = W * np.sqrt(0.6 / np.sqrt(D)) / max(np.sqrt(np.mean((x @ W) ** 2)), 1e-30)
        layers[-1] = (W.astype(np.float32), np.full(len(b), np.sqrt(0.4 / D) if last_bias else 0.0, np.float32))
        w[side] = layers
    csr = (np.concatenate([[0], np.cumsum((R > 0).sum(1))]).astype(np.int64), np.nonzero(R)[1].astype(np.int32), R[R > 0])
    return SimpleNamespace(U=U, I=I, D=D, B=B, R=R, csr=csr, weights=w, max_rating=float(R.max()), lr=0.005, batch=make_batch(B, rs, R),
                           second=make_batch(B, rs, R, second=True))


def names(case):
    return [f"{s[0]}{n}{l}" for s in ("user", "item") for l in range(len(case.weights[s])) for n in "Wb"]


def l2_normalize(x, axis):
    return x * torch.rsqrt(torch.clamp((x * x).sum(axis, keepdim=True), min=1e-12))


class Model:
    def __init__(self, case, similarity, axis="reference", dtype=torch.float64):
        self.case, self.similarity, self.axis, self.dtype = case, similarity, axis, dtype
        self.user_embedding, self.item_embedding = torch.as_tensor(case.R).to(dtype), torch.as_tensor(case.R.T.copy()).to(dtype)
        self.V = [torch.as_tensor(np.asarray(x)).to(dtype).clone() for s in ("user", "item") for Wb in case.weights[s] for x in Wb]
        self.nu = 2 * len(case.weights["user"])
        self.m, self.v, self.step = [np.zeros_like(x.numpy()) for x in self.V], [np.zeros_like(x.numpy()) for x in self.V], 0

    @staticmethod
    def mlp(layers, x):
        for k in range(0, len(layers) - 2, 2):
            x = torch.relu(x @ layers[k] + layers[k + 1])
        return x @ layers[-2] + layers[-1]

    def predict_layer(self, a, b):
        if self.similarity == "dot":
            return (a * b).sum(-1)
        ax = 0 if self.axis == "reference" else -1
        return (l2_normalize(a, ax) * l2_normalize(b, ax)).sum(-1)

    def call(self, V, user, item):
        user_e, item_e = self.user_embedding[user], self.item_embedding[item]
        return self.predict_layer(self.mlp(V[:self.nu], user_e), self.mlp(V[self.nu:], item_e))

    def gradients(self, batch):
        """(loss, y, the gradients in names() order) of train_step."""
        u, i, label = (torch.as_tensor(np.asarray(x)) for x in batch)
        V = [x.clone().requires_grad_(True) for x in self.V]
        output = self.call(V, u.long(), i.long()).reshape(-1)
        t = (label.to(self.dtype) / self.case.max_rating)
        y = torch.clamp(output, EPS, 1 - EPS)
        loss = (-(t * torch.log(y + EPS) + (1 - t) * torch.log(1 - y + EPS))).mean()
        return (loss.detach().double(), output.detach()) + tuple(torch.autograd.grad(loss, V))

    def train_step(self, batch):
        loss, _, *g = self.gradients(batch)
        self.step += 1
        f = self.V[0].numpy().dtype.type
        lr_t = f(adam_lr_t(self.case.lr, self.step))
        for th, m, v, gg in zip(self.V, self.m, self.v, g):                # TF dense ApplyAdam, in place
            gg = gg.numpy()
            m += (gg - m) * f(1 - np.float32(0.9))
            v += (gg * gg - v) * f(1 - np.float32(0.999))
            th.numpy()[...] -= (m * lr_t) / (np.sqrt(v) + f(1e-7))
        return loss

    def get_recs(self, start, stop):
        """get_recs for the chunk of users [start, stop) against all items: [Uc, I]."""
        n, c = stop - start, self.case
        p = self.mlp(self.V[:self.nu], self.user_embedding[start:stop]).unsqueeze(1).expand(n, c.I, c.D)     # the tower of user[k, i] = start + k
        q = self.mlp(self.V[self.nu:], self.item_embedding).unsqueeze(0).expand(n, c.I, c.D)                # ... of item[k, i] = i
        return self.predict_layer(p, q)


def check_exact(case, batch):
    """The properties the bounds rest on: every pre-activation that feeds a ReLU is the same number in float32 and float64."""
    u, i = (torch.as_tensor(np.asarray(x)).long() for x in batch[:2])
    m64, m32 = Model(case, "dot"), Model(case, "dot", dtype=torch.float32)
    for lo, hi, emb, idx in ((0, m64.nu, "user_embedding", u), (m64.nu, len(m64.V), "item_embedding", i)):
        x64, x32 = getattr(m64, emb)[idx], getattr(m32, emb)[idx]
        for k in range(lo, hi - 2, 2):
            z64, z32 = x64 @ m64.V[k] + m64.V[k + 1], x32 @ m32.V[k] + m32.V[k + 1]
            assert torch.equal(z64, z32.double()), "a float32 pre-activation differs from the float64 one"
            x64, x32 = torch.relu(z64), torch.relu(z32)


def check_clip(y64, y32):
    """Every float64 y lies farther from both clip edges than its bound."""
    tol = bound(y64, y32)
    y = np.asarray(y64, np.float64)
    assert (np.abs(y - EPS) > tol).all() and (np.abs(y - (1 - EPS)) > tol).all(), "a y sits on a clip edge"
