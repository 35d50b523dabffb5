"""DMF plugin (YAML key `external.DMF`): Deep Matrix Factorization (Xue et al., IJCAI 2017).

Contract of elliot/recommender/neural/DMF/deep_matrix_factorization.py: hyper-parameters `lr`, `user_mlp`, `item_mlp`, `neg_ratio`,
`reg`, `similarity` with the same file-name shortcuts, result-file name "DMF_...", the point-wise ratio sampler with rating labels,
labels divided by the largest train rating (`max_ratings`), an epoch of transactions * (1 + neg_ratio) samples, the epoch loss handed
to evaluate() as sum / (epoch + 1), users scored in chunks of `batch_size`.

  cosine_axis: reference      `cosine` as the reference writes it, l2_normalize along the batch axis (scores depend on the chunking);
               row            the paper's cosine, along the feature axis.  Ignored for `dot`.
  reg                         accepted and without effect: the reference reads it and it reaches no loss.
  neg_ratio                   an integer >= 1 (the sampler builds `[0] * neg_ratio + [1]`), default 5.
"""
from ast import literal_eval as make_tuple

import numpy as np

from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from ...latent_factor_models.pointwise_plugin import PointwisePluginMixin, RatingLabels
from .deep_matrix_factorization_model import DeepMatrixFactorizationModel


class DMF(PointwisePluginMixin, RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        units = lambda x: [int(v) for v in np.atleast_1d(make_tuple(str(x)))]                      # noqa: E731
        show = lambda x: self._batch_remove(str(x), " []").replace(",", "-")                       # noqa: E731
        self._params_list = [
            param("lr", "lr", 0.0001, read=float, attr="_learning_rate"),
            param("user_mlp", "umlp", "(64,32)", read=units, show=show),
            param("item_mlp", "imlp", "(64,32)", read=units, show=show),
            param("neg_ratio", "negratio", 5),
            param("reg", "reg", 0.001, read=float),
            param("similarity", "sim", "cosine"),
            param("cosine_axis", "cosaxis", "reference"),
        ]
        self.autoset_params()
        if getattr(self._params, "sampler", "philox") == "replay":
            raise Exception("DMF: `sampler: replay` is not offered (the ratio sampler draws another stream than the one replayed)")
        if isinstance(self._neg_ratio, bool) or float(self._neg_ratio) != int(float(self._neg_ratio)) or int(float(self._neg_ratio)) < 1:
            raise Exception(f"DMF: neg_ratio must be an integer >= 1 (the sampler builds [0] * neg_ratio + [1]); got {self._neg_ratio!r}")
        self._neg_ratio = int(float(self._neg_ratio))
        if self._batch_size < 1:
            self._batch_size = self._data.transactions * (1 + self._neg_ratio)
        self._pointwise_setup(neg_ratio=self._neg_ratio)
        self._sampler = RatingLabels(self._sampler, self._ctx, self._data.sp_i_train_ratings)
        self._max_ratings = float(np.max(self._data.sp_i_train_ratings))
        self._model = DeepMatrixFactorizationModel(self._num_users, self._num_items, self._user_mlp, self._item_mlp, self._reg,
                                                   self._similarity, self._max_ratings, self._data.sp_i_train_ratings, self._learning_rate,
                                                   self._seed, ctx=self._ctx, cosine_axis=self._cosine_axis,
                                                   init_weights=kwargs.get("init_weights"))

    def _epoch_events(self):
        return self._data.transactions * (1 + self._neg_ratio)                                    # (deep_matrix_factorization.py:67)

    def _recommendation_block(self):
        return int(self._batch_size)                                                               # get_recs' chunk: the batch-axis norm sees it

    @property
    def name(self):
        return "DMF" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"
