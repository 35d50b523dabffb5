"""FISM_model on the MI355X -- counterpart of elliot/recommender/latent_factor_models/FISM/FISM_model.py.

Gi, Gj [I, F], Bu [U], Bi [I] and one Keras Adam live in HBM (ops.FismDeviceState); every numeric step is a kernel of
libelliot_hip.so (el_fism.hip).  The reference gathers a padded [B, L, F] block of history rows per batch; here a
sample is (user, item) and the user's pooled row is formed once per distinct user of the batch from the CSR history.

Ported as written (the five findings of DESIGN 3.30): the swapped loss arguments (`loss: reference`), the regulariser as a sum with
its unmasked padded slots and batch_predict's unmasked padded slots (`padding: reference`), Keras Adam's sparse apply on every
variable.  Read from TF 2.3, not run -- parity unpinned vs TF.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel

NAMES = ops.FismDeviceState.NAMES


def initial_weights(seed, num_users, num_items, factors):
    """Gi, Gj: RandomUniform(-0.001, 0.001) (:48, :53-54), drawn on the host from the model seed; the biases zero (:50-51).  TF's
    seeded bit stream cannot be reproduced without TF -- the distribution is."""
    rs = np.random.RandomState(seed)
    return {"Gi": rs.uniform(-0.001, 0.001, (num_items, factors)).astype(np.float32),
            "Gj": rs.uniform(-0.001, 0.001, (num_items, factors)).astype(np.float32),
            "Bu": np.zeros(num_users, np.float32), "Bi": np.zeros(num_items, np.float32)}


class FISM_model(DeviceModel):
    def __init__(self, history, factors, lr, alpha, beta, lambda_, gamma, num_users, num_items, random_seed=42, name="FISM", ctx=None,
                 padding="reference", loss="reference", init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self._lr = lr
        w = init_weights if init_weights is not None else initial_weights(random_seed, num_users, num_items, factors)
        self.state = ops.FismDeviceState(self.ctx, w["Gi"], w["Gj"], w["Bu"], w["Bi"], history, alpha=alpha, beta=beta, lambda_=lambda_,
                                         gamma=gamma, padding=padding, loss=loss)
        self._image_version = -1

    def train_step(self, batch):
        """train_step (:78-92).  batch = (user, item, label), shapes [B] or [B, 1]."""
        user, item, label = batch
        y = label if isinstance(label, torch.Tensor) else torch.from_numpy(np.asarray(label, dtype=np.float32))
        y = y.reshape(-1).to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._touch()
        self.state.train_step(self._as_index(user), self._as_index(item), y, self._lr)
        return DeferredLoss(self.state)

    def predict(self, inputs, training=False, **kwargs):
        """The score of (user, item) index arrays of one shape, as batch_predict (:119-144) computes it."""
        user, item = inputs
        shape = tuple(user.shape) if isinstance(user, torch.Tensor) else tuple(np.shape(user))
        return self.state.forward(self._as_index(user), self._as_index(item)).reshape(shape)

    def recommend(self, mask, k, start, stop, item_offset=0):
        """batch_predict + get_top_k for users [start, stop): the user image is rebuilt when the weights changed since it was
        last built, then the fused top-k runs on it."""
        if self._image_version != self._weights_version:
            self._image_version = self._weights_version
            self.state.image()
        return self.state.recommend(self.state._P, start, stop, k, **ops.mask_kwargs(mask))

    # -- checkpoints: the four variables, their Adam slots and the step counter ---------------------------------
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
