"""Slim plugin (YAML key `Slim` / `external.Slim`) -- SLIM: Sparse Linear Methods for Top-N Recommender Systems (Ning & Karypis
2011), in the ElasticNet form of Efficient Top-N Recommendation by Linear Regression (Levy & Jack 2013).

Contract of elliot/recommender/latent_factor_models/Slim/slim.py: hyper-parameters `l1_ratio` (0.001), `alpha` (0.001),
`neighborhood` (10); train() fits one non-negative elastic net per item, builds W once and evaluates.  Extra optional keys:
`exclusion` (`column` | `reference`) and `gpu`.

The reference's train() (slim_model.py:44-110: one sklearn ElasticNet.fit per item) becomes ops.slim_build (el_slim_order,
el_slim_fit, el_slim_w) and ops.knn_score_topk (slim_model.py).  The solver is sklearn's sparse coordinate
descent restated step by step (same visiting order, same float32 updates); it differs from sklearn in the summation order of the
dot products only, and therefore sometimes in the sweep at which a column stops.  Deviations, all documented:
  * `exclusion: column` (the default) zeroes the target's own COLUMN, which is the model of the paper and of the reference's own
    comment ("set the j-th column of X to zero").  The reference does something else: its train matrix is a CSR [U, I], but
    slim_model.py:62-66 uses `train.indptr[currentItem]` as if it were a CSC, so it zeroes the ratings of USER currentItem.  The
    target column stays among the regressors and the fit is the trivial one (every column's largest weight is its own, close
    to 1); with more items than users it raises IndexError; a column whose fit is all zeros would raise in argpartition(-1).
    `exclusion: reference` reproduces that behaviour for parity (ElliotHipError where the reference raises IndexError);
  * a cut that falls inside a tie keeps the smaller index (the reference's argpartition keeps what its introselect happens to);
  * `neighborhood` is limited to 2048 (ElliotHipError beyond);
  * a column without non-zero weights is empty (the reference would raise); the reference's `min(nnz - 1, neighborhood)` is kept;
  * masked items never fill a short list: it is padded with (-1, -inf) where the reference lists -inf items;
  * no dense [U, I] pred_mat is kept: scores are formed and selected per block of users;
  * `name` carries one more field, `excl`, so that two runs that differ only in the exclusion write different files.
Any float ratings work.  save_weights / load_weights pickle W with the hyper-parameters (the reference's get_model_state refers
to an `_A_tilde` that does not exist).
"""
from .... import ops
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .slim_model import SlimModel


class Slim(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (slim.py:54-58), then the exclusion: `name` and every output file name depend on it
        self._params_list = [
            ("_l1_ratio", "l1_ratio", "l1", 0.001, float, None),
            ("_alpha", "alpha", "alpha", 0.001, float, None),
            ("_neighborhood", "neighborhood", "neighborhood", 10, int, None),
            ("_exclusion", "exclusion", "excl", "column", str, None)
        ]
        self.autoset_params()
        if self._exclusion not in ops.SLIM_EXCLUSIONS:
            raise ValueError(f"exclusion {self._exclusion!r} is not supported; supported: {sorted(ops.SLIM_EXCLUSIONS)}")
        self._ratings = self._data.train_dict
        ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = SlimModel(self._data, self._l1_ratio, self._alpha, self._neighborhood, self._seed, self._exclusion, ctx)

    @property
    def name(self):
        return "Slim" \
               + f"_{self.get_base_params_shortcut()}" \
               + f"_{self.get_params_shortcut()}"

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.initialize()                      # no epochs: one evaluation of the built model
        self.evaluate()
