"""Model half of ItemKNN / UserKNN, implementation: standard (item_knn_similarity.py / user_knn_similarity.py: Similarity).

What the reference computes -- a dense similarity, its top-N per column as W, the dense block R.dot(W) / W.dot(R), a masked
top-k per user -- is done on the device without either dense matrix: el_knn_build makes W (exact integer co-occurrence
counts, top-N fused), el_knn_score_topk scores and selects per user in scipy's summation order.
"""
import numpy as np
import scipy.sparse as sp
import torch

from ... import ops
from ..sparse_w_model import SparseWModel


class KnnSimilarity(SparseWModel):
    side = "item"                                   # ItemKNN: similarity of R's columns; UserKNN: of its rows

    def __init__(self, data, num_neighbors, similarity, implicit, ctx):
        if similarity not in ops.KNN_SIMILARITIES:
            raise ValueError(f"Compute Similarity: value for parameter 'similarity' not recognized ({similarity!r}). "
                             f"Supported with implementation: standard: {sorted(ops.KNN_SIMILARITIES)}")
        super().__init__(data, ctx)
        self._num_neighbors = int(num_neighbors)
        self._similarity = similarity
        self._implicit = implicit
        self._preds = None

    def _urm(self):
        m = self._data.sp_i_train if self._implicit else self._data.sp_i_train_ratings
        return sp.csr_matrix(m, dtype=np.float32)

    def _upload_ratings(self):
        R = self._urm()
        if self.side == "user" and not R.has_sorted_indices:      # B operand: rows ascending (the order is immaterial to its sums)
            R = R.copy()
            R.sort_indices()
        super()._upload_ratings(R)

    def _operands(self):
        if self.side == "item":
            return self._R, self._R_vals, self._W, self._W_vals
        return self._W, self._W_vals, self._R, self._R_vals

    def initialize(self):
        self._upload_ratings()
        self._W, self._W_vals = ops.knn_build(self.ctx, self._urm(), self.side, self._num_neighbors, self._similarity)
        self._preds = None

    def recommend(self, mask, k, start, stop):
        if self._preds is None:
            return super().recommend(mask, k, start, stop)
        # restored from a reference checkpoint: its dense block
        block = torch.from_numpy(np.ascontiguousarray(self._preds[start:stop], dtype=np.float32)).to(self.ctx.device)
        return ops.dense_topk(self.ctx, block, start, stop, k, **ops.mask_kwargs(mask))

    def hyper_state(self):
        return {"_similarity": self._similarity, "_num_neighbors": self._num_neighbors, "_implicit": self._implicit}

    def set_hyper_state(self, saving_dict):
        self._similarity = saving_dict["_similarity"]
        self._num_neighbors = saving_dict["_num_neighbors"]
        self._implicit = saving_dict["_implicit"]

    def set_model_state(self, saving_dict):
        if "_preds" in saving_dict:                                  # the reference's checkpoint (get_model_state, :181-187)
            self.set_hyper_state(saving_dict)
            self._preds = np.asarray(saving_dict["_preds"], dtype=np.float32)
            self._W = self._W_vals = None
            return
        super().set_model_state(saving_dict)
        self._preds = None
