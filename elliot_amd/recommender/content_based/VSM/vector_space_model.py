"""VSM plugin (YAML key `VSM` / `external.VSM`) -- Vector Space Model, https://dl.acm.org/doi/10.1145/2362499.2362501 and
https://ieeexplore.ieee.org/document/9143460.

Contract of elliot/recommender/content_based/VSM/vector_space_model.py: hyper-parameters `similarity` (cosine), `user_profile`
and `item_profile` (binary | tfidf, default tfidf), `loader` (ItemAttributes).  A binary user profile is 1 for every feature of
the user's items; a tfidf one is, per feature, the weight in the last item that carries it (attribute_profiles.py).
"""
from ... import attribute_profiles as ap
from .... import ops
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .vector_space_model_similarity import Similarity


class VSM(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (vector_space_model.py:52-57): `name` and every output file name depend on it
        self._params_list = [
            ("_similarity", "similarity", "sim", "cosine", None, None),
            ("_user_profile_type", "user_profile", "up", "tfidf", None, None),
            ("_item_profile_type", "item_profile", "ip", "tfidf", None, None),
            ("_loader", "loader", "load", "ItemAttributes", None, None),
        ]
        self.autoset_params()
        ap.profile_type(self._user_profile_type, "VSM", "user_profile")
        ap.profile_type(self._item_profile_type, "VSM", "item_profile")
        self._side = ap.side_of(self._data, self._loader, "VSM")
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = Similarity(self._data, self.user_profiles, self.item_profiles, self._similarity, self._ctx)

    def user_profiles(self):
        return ap.user_profiles(self._ctx, self._data, self._side, self._user_profile_type, by_len=False)

    def item_profiles(self):
        """build_feature_sparse (ones) or build_feature_sparse_values of the items' TF-IDF rows (:77-89)."""
        tfidf = ap.item_tfidf(self._side.feature_map) if self._item_profile_type == "tfidf" else None
        return ap.sorted_csr(ap.item_features(self._data, self._side, tfidf)[0])

    @property
    def name(self):
        return f"VSM_{self.get_params_shortcut()}"

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.initialize()                      # no epochs: one evaluation of the built model
        self.evaluate()
