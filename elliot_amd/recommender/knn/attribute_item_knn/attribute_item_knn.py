"""AttributeItemKNN plugin (YAML key `AttributeItemKNN` / `external.AttributeItemKNN`) -- MyMediaLite: a free recommender system
library, https://www.researchgate.net/publication/221141162.

Contract of elliot/recommender/knn/attribute_item_knn/attribute_item_knn.py: hyper-parameters `neighbors` (40), `similarity`
(cosine | dot), `implicit`, `loader` (ItemAttributes); the item similarity is taken over the binary item x feature matrix of the
side information, the scores are ItemKNN's R.dot(W).
"""
from ... import attribute_profiles as ap
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from ..attribute_plugin import AttributeKnnPluginMixin
from .attribute_item_knn_similarity import Similarity


class AttributeItemKNN(AttributeKnnPluginMixin, RecMixin, BaseRecommenderModel):
    _similarity_class = Similarity

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (attribute_item_knn.py:47-52): `name` and every output file name depend on it
        self._params_list = [
            ("_num_neighbors", "neighbors", "nn", 40, int, None),
            ("_similarity", "similarity", "sim", "cosine", None, None),
            ("_implicit", "implicit", "bin", False, None, None),
            ("_loader", "loader", "load", "ItemAttributes", None, None),
        ]
        self._init_attribute_knn()

    def attribute_matrix(self):
        """build_feature_sparse (:80-87): ones at (item, feature)."""
        return ap.sorted_csr(ap.item_features(self._data, self._side)[0])

    @property
    def name(self):
        return f"AttributeItemKNN_{self.get_params_shortcut()}"
