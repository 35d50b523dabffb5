"""AttributeUserKNN plugin (YAML key `AttributeUserKNN` / `external.AttributeUserKNN`) -- MyMediaLite: a free recommender system
library, https://www.researchgate.net/publication/221141162.

Contract of elliot/recommender/knn/attribute_user_knn/attribute_user_knn.py: hyper-parameters `neighbors` (40), `similarity`
(cosine | dot), `profile` (binary | tfidf), `implicit`, `loader` (ItemAttributes); the user similarity is taken over the user
profiles over item features (attribute_profiles.py: both quirks of the reference's profiles are kept), the scores are UserKNN's
W.dot(R).
"""
from ... import attribute_profiles as ap
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from ..attribute_plugin import AttributeKnnPluginMixin
from .attribute_user_knn_similarity import Similarity


class AttributeUserKNN(AttributeKnnPluginMixin, RecMixin, BaseRecommenderModel):
    _similarity_class = Similarity

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (attribute_user_knn.py:51-57): `name` and every output file name depend on it
        self._params_list = [
            ("_num_neighbors", "neighbors", "nn", 40, int, None),
            ("_similarity", "similarity", "sim", "cosine", None, None),
            ("_profile_type", "profile", "profile", "binary", None, None),
            ("_implicit", "implicit", "bin", False, None, None),
            ("_loader", "loader", "load", "ItemAttributes", None, None),
        ]
        self._init_attribute_knn()
        ap.profile_type(self._profile_type, "AttributeUserKNN", "profile")

    def attribute_matrix(self):
        """build_feature_sparse_values (:142-151) of the user profiles (:64-73), built on the device."""
        return ap.user_profiles(self._ctx, self._data, self._side, self._profile_type, by_len=True)

    @property
    def name(self):
        return f"AttributeUserKNN_{self.get_params_shortcut()}"
