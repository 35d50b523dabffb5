"""KaHFM plugin (YAML key `external.KaHFM`): knowledge-aware hybrid factorisation machine, per-sample BPR SGD in fp64 over one
factor per knowledge-graph feature.

Contract of elliot/recommender/knowledge_aware/kaHFM/kahfm.py: the six hyper-parameters below with the reference's defaults and
shortcuts (:70-85), `batch_size` forced to 10000 (:108), the factors are the features of the side information (`loader`:
ChainedKG, or ItemAttributes -- only feature_map / features / public_features are read), item rows start as the TF-IDF weights of
their features and user rows as TFIDF.get_profiles gives them (the weight in the LAST item that carries the feature, over the
number of items), `transactions` triplets per epoch, no loss value passed to evaluate() (:161-177).  The start tables are built
by el_kahfm_init; the epoch's triplets are applied in dependency levels as BPRMF applies them, which gives the parameters of the
sequential loop on the same triplet sequence.  Extra optional keys: `sampler` (philox | replay), `hogwild`, `gpu`.
"""
import torch

from .... import ops
from ....dataset.samplers import custom_sampler
from ... import attribute_profiles as ap
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from .kahfm_model import KAHFMModel


class KaHFM(RecMixin, BaseRecommenderModel):
    """Anelli et al., "How to Make Latent Factors Interpretable by Feeding Factorization Machines with Knowledge Graphs", ISWC 2019
    (https://doi.org/10.1007/978-3-030-30793-6_3)."""

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("lr", "lr", 0.05, attr="_learning_rate"),
            param("bias_regularization", "b_reg", 0),
            param("user_regularization", "u_reg", 0.0025),
            param("positive_item_regularization", "pos_i_reg", 0.0025),
            param("negative_item_regularization", "neg_it_reg", 0.00025),
            param("loader", "load", "ChainedKG"),
        ]
        self.autoset_params()
        self._side = ap.side_of(self._data, self._loader, "KaHFM")
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        init_weights = kwargs.get("init_weights")
        if init_weights is None:
            F, w = ap.item_features(self._data, self._side, ap.item_tfidf(self._side.feature_map))
            indptr, indices = ap.train_rows_in_dict_order(self._data)
            P0, Q0 = ops.kahfm_init(self._ctx, indptr, indices, F, w)
            init_weights = (P0, Q0, torch.zeros(Q0.shape[0], dtype=torch.float64, device=Q0.device))
        self._model = KAHFMModel(self._data, init_weights, self._learning_rate, self._user_regularization,
                                 self._bias_regularization, self._positive_item_regularization,
                                 self._negative_item_regularization, ctx=self._ctx,
                                 hogwild=bool(getattr(self._params, "hogwild", False)))
        self._embed_k = self._model.get_factors()
        if getattr(self._params, "sampler", "philox") == "replay":
            self._sampler = custom_sampler.Sampler(self._data.i_train_dict, ctx=self._ctx, replay=True)
        else:
            self._sampler = custom_sampler.Sampler(self._data.sp_i_train, ctx=self._ctx)
        self._batch_size = 10000

    @property
    def name(self):
        return "_".join(["KaHFM", self.get_base_params_shortcut(), self.get_params_shortcut()])

    def _recommendation_block(self):
        return 65536

    def train(self):
        if self._restore:
            return self.restore_weights()
        n = self._data.transactions
        print(f"Transactions: {n}")
        for it in self.iterate(self._epochs):
            print(f"\n********** Iteration: {it + 1}")
            # the reference walks the epoch in batches of 10000 triplets one after the other; one sampler call and one level
            # schedule over the whole epoch apply the same sequence
            for epoch_triplets in self._sampler.step(n, n):
                self._model.train_step(epoch_triplets)
            self.evaluate(it)
