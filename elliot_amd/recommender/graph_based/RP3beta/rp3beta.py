"""RP3beta plugin (YAML key `RP3beta` / `external.RP3beta`) -- Updatable, accurate, diverse, and scalable recommendations for
interactive applications (Paudel et al. 2016, https://doi.org/10.1145/2955101).  `beta: 0` is P3alpha (Cooper et al. 2014).

Contract of elliot/recommender/graph_based/RP3beta/rp3beta.py: hyper-parameters `neighborhood` (10; -1: the number of items),
`alpha` (1.), `beta` (0.6), `normalize_similarity` (False); train() builds the item-item matrix W once and evaluates.  Extra
optional key: `gpu`.

The reference's train() (:77-176) becomes ops.rp3_operands, ops.rp3_build and ops.knn_score_topk (rp3beta_model.py, DESIGN.md
§3.16).  Given the same operands W is the reference's bit for bit wherever no cut falls inside a tie.  Deviations, all documented:
  * a cut that falls inside a tie keeps the smaller index (the reference's argsort keeps what its introsort happens to);
  * `neighborhood` is limited to 2048 after the -1 substitution (ElliotHipError beyond);
  * masked items never fill a short list: it is padded with (-1, -inf) where the reference lists -inf items;
  * no dense [U, I] _preds is kept: scores are formed and selected per block of users.
Any float ratings work: nothing relies on exact sums.  save_weights / load_weights pickle W with the hyper-parameters (the
reference keeps no checkpoint of its own).
"""
from .... import ops
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .rp3beta_model import RP3betaModel


class RP3beta(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (rp3beta.py:26-31): `name` and every output file name depend on it
        self._params_list = [
            ("_neighborhood", "neighborhood", "neighborhood", 10, int, None),
            ("_alpha", "alpha", "alpha", 1., float, None),
            ("_beta", "beta", "beta", 0.6, float, None),
            ("_normalize_similarity", "normalize_similarity", "normalize_similarity", False, bool, None)
        ]
        self.autoset_params()
        if self._neighborhood == -1:
            self._neighborhood = self._data.num_items
        self._ratings = self._data.train_dict
        ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = RP3betaModel(self._data, self._neighborhood, self._alpha, self._beta, self._normalize_similarity, ctx)

    @property
    def name(self):
        return f"RP3beta_{self.get_params_shortcut()}"

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.initialize()                      # no epochs: one evaluation of the built model
        self.evaluate()
