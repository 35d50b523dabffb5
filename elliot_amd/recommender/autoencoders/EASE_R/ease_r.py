"""EASER plugin (YAML key `EASER` / `external.EASER`) -- Embarrassingly Shallow Autoencoders for Sparse Data (Steck 2019,
https://arxiv.org/abs/1905.03375).

Contract of elliot/recommender/autoencoders/EASE_R/ease_r.py: hyper-parameters `neighborhood` (-1: the number of items) and
`l2_norm` (1e3); train() builds the item-item weights B once and evaluates.  `neighborhood` is accepted and named in the file
names, and not used -- the reference sets it (:31-32) and never reads it.  Extra optional key: `gpu`.

The reference's train() (:70-93) becomes el_ease_gram, el_inv_f64, el_ease_weights, and el_csr_dense_scores + el_dense_topk per
block of users (ops.EaseDeviceState).  Deviations, all documented:
  * the inverse is an fp64 LU with partial pivoting, not float32 LAPACK: B agrees with the reference to the reference's own
    float32 error, not bit for bit; given the same B, the scores are the reference's bit for bit;
  * G is exact integer arithmetic: equal to the reference's float32 G while every sum stays below 2^24, exact above;
  * ratings that are neither integers nor half steps are refused (ValueError);
  * masked items never fill a short list: it is padded with (-1, -inf) where the reference lists -inf items;
  * no dense [U, I] _preds is kept: scores are formed and selected per block of users;
  * the device memory G / P, the inverse's right-hand sides, B and one score block need is checked before anything is
    allocated; too little is refused with a ValueError stating the bytes.
save_weights / load_weights pickle B with l2_norm and neighborhood (the reference keeps no checkpoint of its own).
"""
import numpy as np

from .... import ops
from ...device_model import DeviceModel
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin


class EaseModel(DeviceModel):
    """B (float32 [I, I]) and the train ratings on the device; recommend() is the RecMixin scoring hook."""

    def __init__(self, data, l2_norm, neighborhood, ctx):
        self.ctx = ctx
        self._l2_norm = float(l2_norm)
        self._neighborhood = int(neighborhood)
        self.state = ops.EaseDeviceState(ctx, data.sp_i_train_ratings, self._l2_norm)

    def build(self):
        self.state.build()

    def recommend(self, mask, k, start, stop):
        return self.state.recommend(mask, k, start, stop)

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by."""
        return self.state.rank(mask, targets, start, stop)

    def get_model_state(self):
        return {"B": self.state.B.cpu().numpy(), "l2_norm": self._l2_norm, "neighborhood": self._neighborhood}

    def set_model_state(self, saving_dict):
        self._l2_norm = float(saving_dict["l2_norm"])
        self._neighborhood = int(saving_dict["neighborhood"])
        self.state.set_weights(saving_dict["B"])


class EASER(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (ease_r.py:24-27): `name` and every output file name depend on it
        self._params_list = [
            ("_neighborhood", "neighborhood", "neighborhood", -1, int, None),
            ("_l2_norm", "l2_norm", "l2_norm", 1e3, float, None)
        ]
        self.autoset_params()
        if self._neighborhood == -1:
            self._neighborhood = self._data.num_items
        self._ratings = self._data.train_dict
        ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = EaseModel(self._data, self._l2_norm, self._neighborhood, ctx)

    @property
    def name(self):
        return f"EASER_{self.get_params_shortcut()}"

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.build()                           # no epochs: one evaluation of B
        self.evaluate()
