"""Model half of ItemKNN / UserKNN, implementation: standard (item_knn_similarity.py / user_knn_similarity.py: Similarity).

What the reference computes -- a dense similarity, its top-N per column as W, the dense block R.dot(W) / W.dot(R), a masked
top-k per user -- is done on the device without either dense matrix: el_knn_build makes W (exact integer co-occurrence
counts, top-N fused), el_knn_score_topk scores and selects per user in scipy's summation order.
"""
import pickle

import numpy as np
import scipy.sparse as sp
import torch

from ... import ops


class KnnSimilarity(object):
    side = "item"                                   # ItemKNN: similarity of R's columns; UserKNN: of its rows

    def __init__(self, data, num_neighbors, similarity, implicit, ctx):
        if similarity not in ops.KNN_SIMILARITIES:
            raise ValueError(f"Compute Similarity: value for parameter 'similarity' not recognized ({similarity!r}). "
                             f"Supported with implementation: standard: {sorted(ops.KNN_SIMILARITIES)}")
        self._data = data
        self._num_neighbors = int(num_neighbors)
        self._similarity = similarity
        self._implicit = implicit
        self.ctx = ctx
        self._W = self._W_vals = self._preds = None
        self._R = self._R_vals = None

    def _urm(self):
        m = self._data.sp_i_train if self._implicit else self._data.sp_i_train_ratings
        return sp.csr_matrix(m, dtype=np.float32)

    def _upload_ratings(self):
        """R on the device, rows in their stored order (the order scipy sums A's row in)."""
        R = self._urm()
        self._R = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], self.ctx.device)
        self._R_vals = ops.device_values(R.data, self.ctx.device)
        if self.side == "user" and not R.has_sorted_indices:      # B operand: rows ascending (the order is immaterial to its sums)
            R = R.copy()
            R.sort_indices()
            self._R = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], self.ctx.device)
            self._R_vals = ops.device_values(R.data, self.ctx.device)

    def initialize(self):
        self._upload_ratings()
        self._W, self._W_vals = ops.knn_build(self.ctx, self._urm(), self.side, self._num_neighbors, self._similarity)
        self._preds = None

    def recommend(self, mask, k, start, stop):
        """Top-k of users [start, stop) under the tagged mask ("excl" | "cand", DeviceCSR): (idx, val) [n, k] on the device."""
        kind, csr = mask if mask is not None else (None, None)
        excl, cand = (csr if kind == "excl" else None), (csr if kind == "cand" else None)
        if self._preds is not None:                                  # restored from a reference checkpoint: its dense block
            block = torch.from_numpy(np.ascontiguousarray(self._preds[start:stop], dtype=np.float32)).to(self.ctx.device)
            return ops.dense_topk(self.ctx, block, start, stop, k, excl=excl, cand=cand)
        if self.side == "item":
            A, Av, B, Bv = self._R, self._R_vals, self._W, self._W_vals
        else:
            A, Av, B, Bv = self._W, self._W_vals, self._R, self._R_vals
        return ops.knn_score_topk(self.ctx, A, Av, B, Bv, start, stop, k, excl=excl, cand=cand)

    def w_csr(self):
        """W as a host scipy CSR."""
        n = self._W.n_rows
        return sp.csr_matrix((self._W_vals[:self._W.nnz].cpu().numpy(), self._W.indices[:self._W.nnz].cpu().numpy(),
                              self._W.indptr.cpu().numpy()), shape=(n, n))

    def get_model_state(self):
        W = self.w_csr()
        return {"_W_data": W.data, "_W_indices": W.indices, "_W_indptr": W.indptr, "_similarity": self._similarity,
                "_num_neighbors": self._num_neighbors, "_implicit": self._implicit}

    def set_model_state(self, saving_dict):
        self._similarity = saving_dict["_similarity"]
        self._num_neighbors = saving_dict["_num_neighbors"]
        self._implicit = saving_dict["_implicit"]
        if "_preds" in saving_dict:                                  # the reference's checkpoint (get_model_state, :181-187)
            self._preds = np.asarray(saving_dict["_preds"], dtype=np.float32)
            self._W = self._W_vals = None
            return
        self._upload_ratings()
        ip = np.asarray(saving_dict["_W_indptr"], np.int64)
        self._W = ops.DeviceCSR(ip, saving_dict["_W_indices"], ip.shape[0] - 1, self.ctx.device)
        self._W_vals = ops.device_values(saving_dict["_W_data"], self.ctx.device)
        self._preds = None

    def load_weights(self, path):
        with open(path, "rb") as f:
            self.set_model_state(pickle.load(f))

    def save_weights(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.get_model_state(), f)
