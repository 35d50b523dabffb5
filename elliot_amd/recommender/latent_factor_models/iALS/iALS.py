"""iALS plugin (YAML key `iALS` / `external.iALS`) -- Collaborative Filtering for Implicit Feedback Datasets
(http://yifanhu.net/PUB/cf.pdf).

Contract of elliot/recommender/latent_factor_models/iALS/iALS.py: hyper-parameters `factors` (10), `alpha` (1), `epsilon` (1),
`reg` (0.1), `scaling` (linear | log); `epochs` ALS iterations, each followed by evaluate(it).  Extra optional key: `gpu`.
Refused with ValueError: factors > 128, alpha < 0, epsilon <= 0 under log scaling.  Deviations: Cholesky
solves, the dataset is not mutated, no dense pred_mat is kept.
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from ..als_model import IalsModel, check_factors, ials_weights
from ..als_plugin import AlsPluginMixin


class iALS(AlsPluginMixin, RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (iALS.py:49-55): `name` and every output file name depend on it
        self._params_list = [
            ("_factors", "factors", "factors", 10, int, None),
            ("_alpha", "alpha", "alpha", 1, float, None),
            ("_epsilon", "epsilon", "epsilon", 1, float, None),
            ("_reg", "reg", "reg", 0.1, float, None),
            ("_scaling", "scaling", "scaling", "linear", None, None)
        ]
        self.autoset_params()
        self._ratings = self._data.train_dict
        check_factors(self._factors)
        c, w_A, w_b = ials_weights(self._alpha, self._epsilon, self._scaling)
        self._model = IalsModel(self._factors, self._data, self._reg, self._seed, c, w_A, w_b, ctx=self._als_context())

    @property
    def name(self):
        return "iALS" \
               + f"_{self.get_base_params_shortcut()}" \
               + f"_{self.get_params_shortcut()}"
