"""FactorizationMachineModel on the MI355X -- counterpart of elliot/recommender/latent_factor_models/FM/factorization_machine_model.py.

One table E [U + I + nF, F] and one bias vector w in the reference's field order (users, items, features), the global bias g0 and
one Adam live in HBM (ops.FmDeviceState); every numeric step is a kernel of libelliot_hip.so (el_fm.hip).  The
reference is fed a dense one-hot row of width U + I + nF per sample; here a sample is (user, item) and the item's features are
looked up on the device.

`lambda_weights` is accepted and unused, as in the reference: the l2 regulariser handed to the embedding never reaches the tape
loss (train_step does not add self.losses).  The optimiser is TensorFlow's fused dense Adam on every variable (the variables are
read inside tf.map_fn bodies, so their gradients are dense): read from TF 2.3, not run -- parity unpinned vs TF.

Without features (num_features = 0) the reference switches to a biased MF layer with separate tables and the sparse Adam apply; here
the SAME kernels run with empty feature lists.  The function is the same, g0 + w_u + w_i + e_u . e_i; the initial values (one Glorot
limit over the stacked table) and the Adam rounding differ, nothing else does.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel, glorot_uniform

NAMES = ("E", "w", "g0")


def initial_weights(seed, num_users, num_items, num_features, factors):
    """E: GlorotUniform over the shape [N, F] (limit sqrt(6 / (N + F))), drawn on the host from the model seed; w and g0 zero
    (:118-121, :167-170).  TF's seeded bit stream cannot be reproduced without TF -- the distribution is."""
    N = num_users + num_items + num_features
    return {"E": glorot_uniform(np.random.RandomState(seed), N, factors), "w": np.zeros(N, np.float32), "g0": np.zeros(1, np.float32)}


class FactorizationMachineModel(DeviceModel):
    def __init__(self, num_users, num_items, num_features, factors, lambda_weights, learning_rate=0.01, random_seed=42, name="FM",
                 ctx=None, item_features=None, init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self.num_users, self.num_items, self.num_features = num_users, num_items, num_features
        self.factors, self.lambda_weights, self._lr = factors, lambda_weights, learning_rate
        w = init_weights if init_weights is not None else initial_weights(random_seed, num_users, num_items, num_features, factors)
        self.state = ops.FmDeviceState(self.ctx, num_users, num_items, w["E"], w.get("w"), float(np.asarray(w.get("g0", 0.0)).reshape(-1)[0]),
                                       item_features=item_features, n_features=num_features)
        self._image_version = -1

    # -- training ---------------------------------------------------------------------------------------
    def train_step(self, batch):
        """train_step (:62-72).  batch = (user, item, label), shapes [B] or [B, 1]."""
        user, item, label = batch
        y = label if isinstance(label, torch.Tensor) else torch.from_numpy(np.asarray(label, dtype=np.float32))
        y = y.reshape(-1).to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._touch()
        self.state.train_step(self._as_index(user), self._as_index(item), y, self._lr)
        return DeferredLoss(self.state)

    # -- scoring ----------------------------------------------------------------------------------------
    def predict(self, inputs, training=False, **kwargs):
        """predict (:75-83) on (user, item) index arrays of one shape."""
        user, item = inputs
        shape = tuple(user.shape) if isinstance(user, torch.Tensor) else tuple(np.shape(user))
        return self.state.forward(self._as_index(user), self._as_index(item)).reshape(shape)

    get_recs = predict

    def recommend(self, mask, k, start, stop, item_offset=0):
        """get_user_full_array + get_recs + get_top_k for users [start, stop): the item image is rebuilt when the weights changed
        since it was last built, then the fused top-k runs on it."""
        if self._image_version != self._weights_version:
            self._image_version = self._weights_version
            self._scored_version = -1
            self.state.image()
        return self.state.recommend(self.state._Q, self.state._bq, start, stop, k, **ops.mask_kwargs(mask),
                                    items_unchanged=self._items_unchanged())

    # -- checkpoints: the three variables, the Adam slots and the step counter -----------------------------------
    def get_model_state(self):
        d = {"_step": self.state.step, "_g0_master": self.state.g0d.cpu().numpy()}     # (g0 is its float image)
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
        self.state.g0d.copy_(torch.from_numpy(np.ascontiguousarray(d.get("_g0_master", d["g0"]))).reshape(1))
        self.state.step = int(d.get("_step", 0))
