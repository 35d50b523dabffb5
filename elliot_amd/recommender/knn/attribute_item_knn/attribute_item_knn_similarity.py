"""AttributeItemKNN model (attribute_item_knn_similarity.py: Similarity): W over the rows of the binary item x feature matrix,
preds = R.dot(W).  The matrix is binary, so W comes from el_knn_build's exact integer counts, as ItemKNN's does."""
from .... import ops
from ..attribute_knn_similarity import AttributeKnnSimilarity


class Similarity(AttributeKnnSimilarity):
    side = "item"

    def _build_w(self, A):
        return ops.knn_build(self.ctx, A, "user", self._num_neighbors, self._similarity)     # "user": the ROWS of A, the items
