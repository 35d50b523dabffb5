"""ItemKNN model (item_knn_similarity.py: Similarity): W over R's columns, preds = R.dot(W)."""
from ..knn_similarity import KnnSimilarity


class Similarity(KnnSimilarity):
    side = "item"
