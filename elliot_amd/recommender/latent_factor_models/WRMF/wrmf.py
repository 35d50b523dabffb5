"""WRMF plugin (YAML key `WRMF` / `external.WRMF`) -- weighted regularised matrix factorisation
(https://archive.siam.org/meetings/sdm06/proceedings/059zhangs2.pdf).

Contract of elliot/recommender/latent_factor_models/WRMF/wrmf.py: hyper-parameters `factors` (10), `alpha` (1), `reg` (0.1);
`epochs` ALS iterations, each followed by evaluate(it).  The item half uses X^T X of the X the step started from, as the
reference does (wrmf_model.py:42).  Extra optional key: `gpu`.  Refused with ValueError: factors > 128, alpha < 0.
Deviations: Cholesky instead of SuperLU, no dense pred_mat is kept.
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from ..als_model import WrmfModel, check_factors, wrmf_weights
from ..als_plugin import AlsPluginMixin


class WRMF(AlsPluginMixin, RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (wrmf.py:49-53)
        self._params_list = [
            ("_factors", "factors", "factors", 10, None, None),
            ("_alpha", "alpha", "alpha", 1, None, None),
            ("_reg", "reg", "reg", 0.1, None, None)
        ]
        self.autoset_params()
        self._ratings = self._data.train_dict
        check_factors(self._factors)
        c, w_A, w_b = wrmf_weights(self._alpha)
        self._model = WrmfModel(self._factors, self._data, self._reg, self._seed, c, w_A, w_b, ctx=self._als_context())

    @property
    def name(self):
        return "WRMF" \
               + f"_{self.get_base_params_shortcut()}" \
               + f"_{self.get_params_shortcut()}"
