"""SlopeOne plugin (YAML key `SlopeOne` / `external.SlopeOne`) -- Slope One Predictors for Online Rating-Based Collaborative
Filtering (Lemire & Maclachlan 2005, https://arxiv.org/abs/cs/0702144).

Contract of elliot/recommender/algebric/slope_one/slope_one.py: no hyper-parameters, `name == "SlopeOne"`; train() builds freq,
dev and user_mean once and evaluates; `restore` loads a checkpoint -- the reference's own pickle loads here and ours loads
there (keys freq, dev, user_mean).  Extra optional key: `gpu`.

    models:
      SlopeOne:
        meta:
          save_recs: True

Deviations, all documented:
  * freq and dev start from zero (the reference starts them from np.empty);
  * ratings that are neither integers nor half steps are refused (ValueError): the model's sums are exact integers;
  * equal predictions are listed by ascending item index, where the reference's argpartition leaves an arbitrary order;
  * masked items never fill a short list: it is padded with (-1, -inf) and the padding is dropped from the dicts;
  * the device memory freq, dev, the scoring table and one score block need is checked before anything is allocated; too
    little is refused with a ValueError stating the bytes.
"""
from .... import ops
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .slope_one_model import SlopeOneModel


class SlopeOne(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._ratings = self._data.train_dict
        ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = SlopeOneModel(self._data, ctx)

    @property
    def name(self):
        return "SlopeOne"

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.initialize()                      # no epochs: one build of freq, dev and the scoring table
        self.evaluate()
