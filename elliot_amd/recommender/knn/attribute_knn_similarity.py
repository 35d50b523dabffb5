"""Model half shared by AttributeItemKNN and AttributeUserKNN (attribute_item_knn_similarity.py /
attribute_user_knn_similarity.py: Similarity): ItemKNN / UserKNN whose similarity is taken over the rows of an attribute matrix
instead of the ratings.  Scores, masks, top-k and checkpoints are KnnSimilarity's."""
from .knn_similarity import KnnSimilarity


class AttributeKnnSimilarity(KnnSimilarity):

    def __init__(self, data, attribute_matrix, num_neighbors, similarity, implicit, ctx):
        """attribute_matrix: a function without arguments that returns the scipy CSR whose rows are the targets -- called by
        initialize() only, so a restored model never builds it."""
        super().__init__(data, num_neighbors, similarity, implicit, ctx)
        self._attribute_matrix = attribute_matrix

    def _build_w(self, A):
        raise NotImplementedError

    def initialize(self):
        self._upload_ratings()
        self._W, self._W_vals = self._build_w(self._attribute_matrix())
        self._preds = None
