"""AttributeUserKNN model (attribute_user_knn_similarity.py: Similarity): W over the rows of the float-valued user profile
matrix (el_knn_build_f32: fp64 sums in a fixed order), preds = W.dot(R) with UserKNN's reverse-neighbour semantics."""
from .... import ops
from ..attribute_knn_similarity import AttributeKnnSimilarity


class Similarity(AttributeKnnSimilarity):
    side = "user"

    def _build_w(self, A):
        return ops.knn_build_f32(self.ctx, A, self._num_neighbors, self._similarity)
