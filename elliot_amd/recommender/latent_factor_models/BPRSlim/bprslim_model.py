"""BPRSlimModel on the device -- counterpart of elliot/recommender/latent_factor_models/BPRSlim/bprslim_model.py.

The reference's model is a dense float64 item-item matrix S trained by one Python loop per (triplet, seen item) (train_step,
:36-67) and scored by one per (user, item, seen item) (predict, :69-84).  Here train_step is el_bprslim_apply over dependency
levels of the triplet sequence -- a triplet reads and writes rows i and j of S, so two triplets that share neither run in one
launch -- and predict + get_user_recs are el_bprslim_scores + el_dense_topk_f64 per block of users (ops.BprSlimDeviceState,
DESIGN.md §3.23).  Given S, every prediction equals the reference's bit for bit; a trained S differs from the reference's by the
order in which a triplet's sum over the seen items is taken, and by nothing else.

S STARTS FROM ZERO.  The reference starts it from np.empty and relies on fresh pages being zero.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeviceModel


class BPRSlimModel(DeviceModel):
    """S and its scoring table on the device; recommend() is the RecMixin scoring hook."""

    def __init__(self, data, lr, lj_reg, li_reg, ctx):
        self.ctx = ctx
        self._data = data
        self.state = ops.BprSlimDeviceState(ctx, data.sp_i_train_ratings, lr, li_reg, lj_reg)
        self.levels_last = 0

    def train_step(self, batch):
        """train_step (:36-67) for every triplet of the batch, one after the other in the order given; arrays of shape [B] or
        [B, 1], host or device.  Returns the sum of the triplets' losses x_uij ** 2, added in fp64 in that order."""
        u, i, j = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in batch)
        self.levels_last, x = self.state.apply_sequential_equivalent(u, i, j)
        return float(np.cumsum(x * x)[-1]) if x.shape[0] else 0.0

    def recommend(self, mask, k, start, stop):
        return self.state.recommend(mask, k, start, stop)

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by."""
        return self.state.rank(mask, targets, start, stop)

    def get_model_state(self):
        """The reference's one key: `_s_dense`, a float64 [I, I] ndarray."""
        return {"_s_dense": self.state.S.cpu().numpy()}

    def set_model_state(self, saving_dict):
        self.state.set_model(saving_dict["_s_dense"])
