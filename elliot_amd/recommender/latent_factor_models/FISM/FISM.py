"""FISM plugin (YAML key `external.FISM`): Factored Item Similarity Models (Kabbur, Ning, Karypis, KDD 2013).

Contract of elliot/recommender/latent_factor_models/FISM/FISM.py: hyper-parameters `factors`, `lr`, `alpha` (clamped to [0, 1]),
`beta`, `lambda`, `gamma`, `neg_ratio`, result-file name "FISM_...", point-wise samples in batches of `batch_size` whose label is the
RATING of a positive and 0 for a negative, a positive with probability 1 / (neg_ratio + 1) (pointwise_pos_neg_ratio_ratings_sampler),
epoch loss handed to evaluate() as sum / (epoch + 1).

Ported as written, each switchable here:
  loss: reference | bce       `self.loss(output, label)` calls Keras BinaryCrossentropy with its arguments swapped; `bce` is the
                              cross-entropy that was meant.
  padding: reference | none   the padded slots of the history matrix (item id 0) are not masked out of the regulariser nor out of
                              batch_predict's sum; `none` drops both.
  neg_ratio                   must be an integer (the sampler builds `[0] * neg_ratio + [1]`; the reference's own default 0.5 raises
                              a TypeError): a non-integer is refused, the default is 1.
get_recommendations calls predict(offset, offset_stop), which cannot run; batch_predict is what is scored here.  `sampler: replay` is
not offered: the ratio sampler interleaves np.random.shuffle with its draws, another stream than the one replayed for MF.
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from ..pointwise_plugin import PointwisePluginMixin, RatingLabels
from .FISM_model import FISM_model


class FISM(PointwisePluginMixin, RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("factors", "factors", 100, read=int),
            param("lr", "lr", 0.001, read=float),
            param("beta", "beta", 0.001, read=float),
            param("lambda", "lambda", 0.001, read=float),
            param("gamma", "gamma", 0.001, read=float),
            param("alpha", "alpha", 0.5, read=lambda x: min(max(0.0, float(x)), 1.0)),
            param("neg_ratio", "neg_ratio", 1),
            param("padding", "padding", "reference"),
            param("loss", "loss", "reference", attr="_loss_kind"),
        ]
        self.autoset_params()
        if getattr(self._params, "sampler", "philox") == "replay":
            raise Exception("FISM: `sampler: replay` is not offered (the ratio sampler draws another stream than the one replayed)")
        if isinstance(self._neg_ratio, bool) or float(self._neg_ratio) != int(float(self._neg_ratio)) or int(float(self._neg_ratio)) < 1:
            raise Exception(f"FISM: neg_ratio must be an integer >= 1 (the sampler builds [0] * neg_ratio + [1]); got {self._neg_ratio!r}")
        self._neg_ratio = int(float(self._neg_ratio))
        self._pointwise_setup(neg_ratio=self._neg_ratio)
        self._sampler = RatingLabels(self._sampler, self._ctx, self._data.sp_i_train_ratings)
        train = self._data.sp_i_train.tocsr()
        self._model = FISM_model((train.indptr, train.indices), self._factors, self._lr, self._alpha, self._beta, self._lambda,
                                 self._gamma, self._num_users, self._num_items, self._seed, ctx=self._ctx, padding=self._padding,
                                 loss=self._loss_kind, init_weights=kwargs.get("init_weights"))

    @property
    def name(self):
        return "FISM" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"
