"""UserKNN plugin (YAML key `UserKNN` / `external.UserKNN`) -- GroupLens: An Open Architecture for Collaborative Filtering
of Netnews, https://dl.acm.org/doi/10.1145/192844.192905.

Contract of elliot/recommender/knn/user_knn/user_knn.py: the hyper-parameters of ItemKNN; the similarity is taken over
users, and a user's scores sum the rating rows of the users whose top-N hold it (W.dot(R), user_knn_similarity.py:77).
"""
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from ..knn_plugin import KnnPluginMixin
from .user_knn_similarity import Similarity


class UserKNN(KnnPluginMixin, RecMixin, BaseRecommenderModel):
    _similarity_class = Similarity

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._init_knn()

    @property
    def name(self):
        return f"UserKNN_{self.get_params_shortcut()}"
