"""ItemKNN plugin (YAML key `ItemKNN` / `external.ItemKNN`) -- Amazon.com recommendations: item-to-item collaborative
filtering, http://ieeexplore.ieee.org/document/1167344/.

Contract of elliot/recommender/knn/item_knn/item_knn.py: hyper-parameters `neighbors` (40), `similarity` (cosine | dot),
`implementation` (standard only), `implicit` (False: the ratings, True: the binary train matrix); the aiolli options are
accepted, named in the file names, and ignored with the reference's message.
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from ..knn_plugin import KnnPluginMixin
from .item_knn_similarity import Similarity


class ItemKNN(KnnPluginMixin, RecMixin, BaseRecommenderModel):
    _similarity_class = Similarity

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._init_knn()

    @property
    def name(self):
        return f"ItemKNN_{self.get_params_shortcut()}"
