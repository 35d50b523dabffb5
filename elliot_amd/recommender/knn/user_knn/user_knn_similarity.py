"""UserKNN model (user_knn_similarity.py: Similarity): W over R's rows, preds = W.dot(R) -- a sum over the users whose
top-N hold u (reverse neighbours), as the reference computes it."""
from ..knn_similarity import KnnSimilarity


class Similarity(KnnSimilarity):
    side = "user"
