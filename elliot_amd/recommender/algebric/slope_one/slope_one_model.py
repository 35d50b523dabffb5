"""SlopeOneModel on the device (Lemire & Maclachlan 2005, https://arxiv.org/abs/cs/0702144).

The reference's model (elliot/recommender/algebric/slope_one/slope_one_model.py) is a triple Python loop over every co-rated
pair (initialize) and a Python comprehension per (user, item) (predict).  Here initialize is el_slope_build -- the integer
co-occurrence expansion with two counters per cell -- and predict + get_user_recs are el_slope_scores + el_dense_topk_f64 per
block of users (ops.SlopeDeviceState).  With integer or half-step ratings every sum of the model is exact, so
freq, dev, user_mean and every prediction equal the reference's bit for bit.

freq and dev START FROM ZERO.  The reference starts them from np.empty and relies on fresh pages being zero.
"""
import numpy as np

from .... import ops
from ...device_model import DeviceModel
from ...attribute_profiles import train_rows_in_dict_order


class SlopeOneModel(DeviceModel):
    """freq, dev, user_mean and the scoring table on the device; recommend() is the RecMixin scoring hook."""

    def __init__(self, data, ctx):
        self.ctx = ctx
        self._data = data
        self.state = ops.SlopeDeviceState(ctx, data.sp_i_train_ratings, train_rows_in_dict_order(data))

    def initialize(self):
        self.state.build()

    def recommend(self, mask, k, start, stop):
        return self.state.recommend(mask, k, start, stop)

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by."""
        return self.state.rank(mask, targets, start, stop)

    def get_model_state(self):
        """The reference's keys and types: freq and dev float64 [I, I] arrays (dev with -0.0 below the diagonal wherever +0.0
        stands above it), user_mean a list of np.float64."""
        return {"freq": self.state.freq.cpu().numpy().astype(np.float64), "dev": self.state.dev.cpu().numpy(),
                "user_mean": [np.float64(x) for x in self.state.user_mean_host]}

    def set_model_state(self, saving_dict):
        self.state.set_model(saving_dict["freq"], saving_dict["dev"], saving_dict["user_mean"])
