"""NAIS plugin (YAML key `external.NAIS`): Neural Attentive Item Similarity (He et al., TKDE 2018), `algorithm: concat`.

Contract of elliot/recommender/neural/NAIS/nais.py: hyper-parameters `factors`, `algorithm`, `weight_size`, `lr`, `l_w`, `l_b`, `alpha`
(clamped to [0, 1]), `beta`, `neg_ratio`, result-file name "NAIS_...", FISM's point-wise ratio sampler with rating labels, epoch loss
handed to evaluate() as sum / (epoch + 1).

  algorithm: concat           `product` is refused by name: its first layer does not split into a history and a target half.
  l_w                         accepted and without effect: the reference reads it and never uses it.
  loss, padding               FISM's switches (`reference` | `bce`, `reference` | `none`).
  neg_ratio                   an integer >= 1 (the sampler builds `[0] * neg_ratio + [1]`), default 1.
get_recommendations scores blocks of users through el_nais_scores + el_dense_topk.
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from ...latent_factor_models.pointwise_plugin import PointwisePluginMixin, RatingLabels
from .nais_model import NAIS_model


class NAIS(PointwisePluginMixin, RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("factors", "factors", 100, read=int),
            param("algorithm", "algorithm", "concat"),
            param("weight_size", "weight_size", 32, read=int),
            param("lr", "lr", 0.001, read=float),
            param("l_w", "l_w", 0.001, read=float),
            param("l_b", "l_b", 0.001, read=float),
            param("alpha", "alpha", 0.5, read=lambda x: min(max(0.0, float(x)), 1.0)),
            param("beta", "beta", 0.5, read=float),
            param("neg_ratio", "neg_ratio", 1),
            param("padding", "padding", "reference"),
            param("loss", "loss", "reference", attr="_loss_kind"),
        ]
        self.autoset_params()
        if self._algorithm != "concat":
            raise Exception(f"NAIS: algorithm {self._algorithm!r} is not offered: only `concat` runs here (`product` needs a batched "
                            "matrix kernel of its own)")
        if getattr(self._params, "sampler", "philox") == "replay":
            raise Exception("NAIS: `sampler: replay` is not offered (the ratio sampler draws another stream than the one replayed)")
        if isinstance(self._neg_ratio, bool) or float(self._neg_ratio) != int(float(self._neg_ratio)) or int(float(self._neg_ratio)) < 1:
            raise Exception(f"NAIS: neg_ratio must be an integer >= 1 (the sampler builds [0] * neg_ratio + [1]); got {self._neg_ratio!r}")
        self._neg_ratio = int(float(self._neg_ratio))
        self._pointwise_setup(neg_ratio=self._neg_ratio)
        self._sampler = RatingLabels(self._sampler, self._ctx, self._data.sp_i_train_ratings)
        train = self._data.sp_i_train.tocsr()
        self._model = NAIS_model((train.indptr, train.indices), self._algorithm, self._weight_size, self._factors, self._lr, self._l_w,
                                 self._l_b, self._alpha, self._beta, self._num_users, self._num_items, self._seed, ctx=self._ctx,
                                 padding=self._padding, loss=self._loss_kind, init_weights=kwargs.get("init_weights"))

    @property
    def name(self):
        return "NAIS" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"
