"""NAIS_model on the MI355X -- counterpart of elliot/recommender/neural/NAIS/nais_model.py, `algorithm: concat`.

Gi, Gj [I, F], Bu [U], Bi [I], the three Dense layers W1 [2F, 2F], b1, W2 [2F, Ws], b2, W3 [Ws, 1], b3 and one Keras Adam live in HBM
(ops.NaisDeviceState); every numeric step is a kernel of libelliot_hip.so (el_nais.hip).  The reference gathers a padded
[B, L, 2F] block per batch and a [users, I, L, 2F] block per scored user block; here the first layer is split into a history half and a
target half (one product each per call) and every (history row, target) pair is recomputed where it is needed.

Ported as written: FISM's swapped loss arguments (`loss: reference`), the summed regulariser with its unmasked padded
slots and batch_predict's unmasked padded slots (`padding: reference`), exp() without a subtracted maximum, `l_w` read and never used,
Keras Adam on every variable.  Read from TF 2.3, not run -- parity unpinned vs TF.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel

NAMES = ops.NaisDeviceState.NAMES


def initial_weights(seed, num_users, num_items, factors, weight_size):
    """Embeddings and Dense kernels: RandomUniform(-0.001, 0.001) (:52-72), drawn from the seeded torch generator; every bias zero.
    TF's seeded bit stream cannot be reproduced without TF -- the distribution is."""
    gen = torch.Generator().manual_seed(int(seed))
    draw = lambda *s: ((torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1) * 0.001).float().numpy()      # noqa: E731
    f2 = 2 * factors
    return {"Gi": draw(num_items, factors), "Gj": draw(num_items, factors), "Bu": np.zeros(num_users, np.float32),
            "Bi": np.zeros(num_items, np.float32), "W1": draw(f2, f2), "b1": np.zeros(f2, np.float32), "W2": draw(f2, weight_size),
            "b2": np.zeros(weight_size, np.float32), "W3": draw(weight_size), "b3": np.zeros(1, np.float32)}


class NAIS_model(DeviceModel):
    def __init__(self, history, algorithm, weight_size, factors, lr, l_w, l_b, alpha, beta, num_users, num_items, random_seed=42, name="NAIS",
                 ctx=None, padding="reference", loss="reference", init_weights=None, **kwargs):
        if algorithm != "concat":
            raise Exception(f"NAIS: algorithm {algorithm!r} is not offered: only `concat` splits into a history and a target half "
                            "(`product` needs a batched matrix kernel of its own, DESIGN 3.31)")
        self.ctx = ctx or ops.get_context(0)
        self._lr, self._l_w = lr, l_w                                                   # (l_w: read by the reference, used nowhere)
        w = init_weights if init_weights is not None else initial_weights(random_seed, num_users, num_items, factors, weight_size)
        self.state = ops.NaisDeviceState(self.ctx, w, history, alpha=alpha, beta=beta, l_b=l_b, padding=padding, loss=loss)

    def train_step(self, batch):
        """train_step (:152-166).  batch = (user, item, label), shapes [B] or [B, 1]."""
        user, item, label = batch
        y = label if isinstance(label, torch.Tensor) else torch.from_numpy(np.asarray(label, dtype=np.float32))
        y = y.reshape(-1).to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._touch()
        self.state.train_step(self._as_index(user), self._as_index(item), y, self._lr)
        return DeferredLoss(self.state)

    def predict(self, inputs, training=False, **kwargs):
        """The score of (user, item) index arrays of one shape, as batch_predict (:194-219) computes it."""
        user, item = inputs
        shape = tuple(user.shape) if isinstance(user, torch.Tensor) else tuple(np.shape(user))
        return self.state.forward(self._as_index(user), self._as_index(item)).reshape(shape)

    def recommend(self, mask, k, start, stop, item_offset=0):
        """batch_predict + get_top_k for users [start, stop): the dense block of el_nais_scores, then el_dense_topk."""
        return self.state.recommend(start, stop, k, **ops.mask_kwargs(mask))

    # -- checkpoints: the ten variables, their Adam slots and the step counter ----------------------------------
    def get_model_state(self):
        d = {"_step": self.state.step}
        for n in NAMES:
            for pre in ("", "m", "v"):
                d[pre + n] = getattr(self.state, pre + n).cpu().numpy()
        return d

    def set_model_state(self, d):
        self._touch()
        for n in NAMES:
            for pre in ("", "m", "v"):
                if pre + n in d:
                    t = getattr(self.state, pre + n)
                    t.copy_(torch.from_numpy(np.ascontiguousarray(d[pre + n])).reshape(t.shape))
        self.state.step = int(d.get("_step", 0))
