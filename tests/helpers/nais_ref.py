"""Torch-CPU restatement of NAIS_model (elliot/recommender/neural/NAIS/nais_model.py, `algorithm: concat`) for the NAIS tests, in the
dtype of the model (float64 = the reference value, float32 = the yardstick of bound).

A literal transcription of `attention` + `softmax` + `call` (:79-150), `train_step` (:152-166, gradients from autograd) and
`batch_predict` (:194-219): the padded history matrix and its mask, the concatenated [B, L, 2F] MLP input through three Dense layers,
exp() without a subtracted maximum, the mask applied in `call` and NOT in batch_predict, the loss called as loss(output, label), the
regulariser over the unmasked source.  It shares no first-layer split, no collapsed w = W2 W3 and no hand-derived gradient with
el_nais.hip.  pad / loss are fism_ref's switches.  batch_predict evaluates a user's L - n padded slots (identical rows of item 0) once
and counts them L - n times.  Profile, batches, bound and distance come from fism_ref (U = I = 600, L = 515).

make_case(dyadic=True) draws Gi, Gj, W1, b1 as integers in [-8, 8] times 2^-4: every first-layer pre-activation is then exact in
float32 in any summation order, so no ReLU falls on another side of zero in float32 than in float64 (check_exact asserts it bit for
bit, and that the float64 logits stay inside [-4, 4]: W2, W3, b2, b3 are ordinary floats scaled for that).
"""
import numpy as np
import torch

from oracle.bprmf_batch import adam_tf_sparse_apply
from tests.helpers import fism_ref
from tests.helpers.fism_ref import EPS, bound, distance, l2_loss  # noqa: F401

NAMES = ("Gi", "Gj", "Bu", "Bi", "W1", "b1", "W2", "b2", "W3", "b3")


def piece_counts(lens, piece):
    """Whether lists of these lengths are cut into one piece, 2 .. 16 pieces, more than 16 pieces."""
    n = np.maximum(1, -(-np.asarray(lens) // piece))
    return bool((n == 1).any()), bool(((n >= 2) & (n <= 16)).any()), bool((n > 16).any())


def make_case(F, B, Ws=32, alpha=0.5, beta=0.5, dyadic=True, uniform=False):
    """fism_ref's case with the MLP on top.  uniform: W3 = 0, b3 = 0 -- the attention is uniform and the model is FISM."""
    c = fism_ref.make_case(F, B, alpha)
    rs = np.random.RandomState(77 * F + B + Ws)
    dy = (lambda *s: rs.randint(-8, 9, s).astype(np.float32) / 16) if dyadic else (lambda *s: rs.uniform(-0.3, 0.3, s).astype(np.float32))
    c.Gi, c.Gj, c.W1, c.b1 = dy(c.I, F), dy(c.I, F), dy(2 * F, 2 * F), dy(2 * F)
    W2, W3, b2 = rs.uniform(-1, 1, (2 * F, Ws)), rs.uniform(-1, 1, Ws), rs.uniform(-1, 1, Ws)
    W3 *= 3.5 / ((F / 2 + 0.5) * np.abs(W2 @ W3).sum())                               # |v| <= F / 2 + 1 / 2, so |relu(v) . w| <= 3.5
    b2 *= 0.3 / max(abs(b2 @ W3), 1e-30)
    c.W2, c.b2, c.W3, c.b3 = W2.astype(np.float32), b2.astype(np.float32), W3.astype(np.float32), rs.uniform(-0.2, 0.2, 1).astype(np.float32)
    if uniform:
        c.W3, c.b3 = np.zeros_like(c.W3), np.zeros_like(c.b3)
    c.Ws, c.beta_smooth, c.l_b = Ws, beta, 0.02
    return c


class Model(fism_ref.Model):
    def __init__(self, case, dtype=torch.float64, pad=True, loss="reference"):
        super().__init__(case, dtype, pad, loss)
        for n in NAMES:
            setattr(self, n, torch.as_tensor(getattr(case, n)).to(dtype).clone())
        self.m = {n: np.zeros_like(getattr(self, n).numpy()) for n in NAMES}
        self.v = {n: np.zeros_like(getattr(self, n).numpy()) for n in NAMES}

    def first(self, V, x):
        return x @ V[4] + V[5]                                                        # Dense(2F): the pre-activation

    def mlp(self, V, x):
        return ((torch.relu(self.first(V, x)) @ V[6] + V[7]) @ V[8].reshape(-1, 1) + V[9]).squeeze(-1)

    def attend(self, V, user_history, target, coef, user_bias, item_bias, weight):
        """attention + softmax over slots that count `weight` times (the mask in call, the multiplicities in batch_predict)."""
        similarity = torch.matmul(user_history, target.unsqueeze(2)).squeeze(2)
        mlp_input = torch.cat([user_history, target.unsqueeze(1).expand(-1, user_history.shape[1], -1)], 2)
        exp_logits = weight * torch.exp(self.mlp(V, mlp_input))
        weights = exp_logits / exp_logits.sum(1, keepdim=True) ** self.case.beta_smooth
        return 1 / (1 + torch.exp(-(coef * (weights * similarity).sum(1) + user_bias + item_bias)))

    def chunk_loss(self, V, user, item, label, B):
        c, mask = self.case, self.mask[user]
        source, target, user_bias, item_bias = V[0][self.hist[user]], V[1][item], V[2][user], V[3][item]
        output = self.attend(V, source, target, self.coef[user], user_bias, item_bias, mask)
        if not self.pad:
            source = source * mask.unsqueeze(2)
        reg = c.l_b * l2_loss(user_bias) + c.l_b * l2_loss(item_bias) + l2_loss(source) + l2_loss(target)
        label = torch.as_tensor(label, dtype=torch.float64)
        if self.loss_kind == "reference":
            y_true, y_pred = output.double(), torch.clamp(label, EPS, 1 - EPS)
        else:
            y_true, y_pred = (label > 0).to(self.dtype), torch.clamp(output, EPS, 1 - EPS)
        bce = y_true * torch.log(y_pred + EPS) + (1 - y_true) * torch.log(1 - y_pred + EPS)
        return (-bce).sum().double() / B + reg.double()

    def gradients(self, batch, chunk=128):
        """(loss, the ten gradients in NAMES order) of train_step."""
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
            adam_tf_sparse_apply(getattr(self, n).numpy(), self.m[n], self.v[n], gg.numpy(), lr, self.step)
        return loss

    def batch_predict(self, users, chunk=100):
        """batch_predict for these users against ALL items, user by user: [len(users), I]."""
        V, c, out = tuple(getattr(self, n) for n in NAMES), self.case, []
        for u in users:
            n = len(c.hist[u])
            slots = torch.cat([self.hist[u, :n], torch.zeros(1, dtype=torch.int64)]) if self.pad and n < c.L else self.hist[u, :n]
            weight = torch.ones(len(slots), dtype=self.dtype)
            weight[n:] = c.L - n
            rows = []
            for s in range(0, c.I, chunk):
                item = torch.arange(s, min(s + chunk, c.I))
                hist = self.Gi[slots].unsqueeze(0).expand(len(item), -1, -1)
                rows.append(self.attend(V, hist, self.Gj[item], self.coef[u], self.Bu[u], self.Bi[item], weight))
            out.append(torch.cat(rows))
        return torch.stack(out)


def check_exact(case, batch):
    """The two properties the gradient bound rests on, for every (sample, slot) of the batch."""
    u, i = (torch.as_tensor(np.asarray(x).astype(np.int64)) for x in batch[:2])
    m64, m32 = Model(case, torch.float64), Model(case, torch.float32)
    for s in range(0, len(u), 128):
        pre = []
        for m in (m64, m32):
            V = tuple(getattr(m, n) for n in NAMES)
            h, t = m.Gi[m.hist[u[s:s + 128]]], m.Gj[i[s:s + 128]]
            x = torch.cat([h, t.unsqueeze(1).expand(-1, h.shape[1], -1)], 2)
            pre.append((m.first(V, x), m.mlp(V, x)))
        assert torch.equal(pre[0][0], pre[1][0].double()), "a float32 pre-activation differs from the float64 one"
        assert float(pre[0][1].abs().max()) <= 4.0, "a float64 logit is outside [-4, 4]"
