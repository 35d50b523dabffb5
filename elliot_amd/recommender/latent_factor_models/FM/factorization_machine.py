"""FM plugin (YAML key `external.FM`): Factorization Machines (Rendle, https://ieeexplore.ieee.org/document/5694074) over users,
items and the items' attributes.

Contract of elliot/recommender/latent_factor_models/FM/factorization_machine.py:25-164: hyper-parameters `factors`, `lr`, `reg`,
`loader` (the side-information namespace, default "ItemAttributes"), result-file name "FM_...", point-wise samples in batches of
`batch_size` whose label is the RATING of a positive and 0 for a negative (pointwise_pos_neg_ratings_sampler), epoch loss handed
to evaluate() as sum / (epoch + 1) (:119).  `reg` is accepted, named in the result file and has no effect, as in the reference (the
regulariser never reaches the tape loss).  The item's features are its `feature_map` entries through `public_features`
(get_item_fragment, :127-141) -- a set; an item may have none.  Without the loader, or without `nfeatures`, the same kernels run
with no feature rows (the reference's biased-MF fallback, :75-76).

The sampler is the device philox sampler of the point-wise plugins (its coin is turned into the label by el_fm_labels);
`sampler: replay` is not offered: the reference's FM sampler interleaves np.random.shuffle with its draws, another stream than the
one replayed for MF.  The training loop is RecMixin.train(); lists come from the item image and the fused top-k instead of one
[I, U + I + nF] block per user (:143-164).
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from ..pointwise_plugin import PointwisePluginMixin, RatingLabels as _RatingLabels
from .factorization_machine_model import FactorizationMachineModel


class FM(PointwisePluginMixin, RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("factors", "factors", 10, read=int),
            param("lr", "lr", 0.001, read=float, attr="_learning_rate"),
            param("reg", "reg", 0.1, read=float, attr="_l_w"),
            param("loader", "load", "ItemAttributes"),
        ]
        self.autoset_params()
        if getattr(self._params, "sampler", "philox") == "replay":
            raise Exception("FM: `sampler: replay` is not offered (the reference's FM sampler draws another stream than the one replayed)")
        self._pointwise_setup()
        self._sampler = _RatingLabels(self._sampler, self._ctx, self._data.sp_i_train_ratings)
        self._side = getattr(self._data.side_information, self._loader, None)
        if hasattr(self._side, "nfeatures") and hasattr(self._side, "feature_map"):
            self._nfeatures = int(self._side.nfeatures)
            self._item_features = self.get_item_features()
        else:
            self._nfeatures, self._item_features = 0, None
        self._model = FactorizationMachineModel(self._num_users, self._num_items, self._nfeatures, self._factors, self._l_w,
                                                self._learning_rate, self._seed, ctx=self._ctx, item_features=self._item_features,
                                                init_weights=kwargs.get("init_weights"))

    def get_item_features(self):
        """get_item_fragment (:127-141) without the one-hot block: per private item the private ids of its features."""
        pub, fmap = self._side.public_features, self._side.feature_map
        return [sorted({pub[f] for f in fmap[self._data.private_items[item]]}) for item in range(self._num_items)]

    @property
    def name(self):
        return "FM" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"
