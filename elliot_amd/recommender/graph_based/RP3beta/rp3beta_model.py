"""Model half of RP3beta (rp3beta.py: train, get_user_predictions).

What the reference computes -- two normalised operands, the dense item-item product in blocks of 200 rows, a cut of every row
and of every column, the block R.dot(W), a masked top-k per user -- is done on the device without the dense product and without
the [U, I] score block: ops.rp3_operands (el_csr_row_l1; the two powers stay NumPy's, on the host), ops.rp3_build (el_rp3_rows,
el_rp3_cut) and ops.knn_score_topk per block of users.
"""
import pickle

import numpy as np
import scipy.sparse as sp

from .... import ops


class RP3betaModel(object):

    def __init__(self, data, neighborhood, alpha, beta, normalize_similarity, ctx):
        self._data = data
        self._neighborhood = int(neighborhood)
        self._alpha = float(alpha)
        self._beta = float(beta)
        self._normalize_similarity = bool(normalize_similarity)
        self.ctx = ctx
        self._W = self._W_vals = self._R = self._R_vals = None

    def _urm(self):
        return sp.csr_matrix(self._data.sp_i_train_ratings, dtype=np.float32)

    def _upload_ratings(self):
        """R on the device, rows in their stored order (the order scipy sums A's row in)."""
        R = self._urm()
        self._R = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], self.ctx.device)
        self._R_vals = ops.device_values(R.data, self.ctx.device)

    def initialize(self):
        self._upload_ratings()
        operands = ops.rp3_operands(self.ctx, self._urm(), self._alpha, self._beta)
        self._W, self._W_vals = ops.rp3_build(self.ctx, *operands, self._neighborhood, self._normalize_similarity)

    def recommend(self, mask, k, start, stop):
        """Top-k of users [start, stop) under the tagged mask ("excl" | "cand", DeviceCSR): (idx, val) [n, k] on the device."""
        kind, csr = mask if mask is not None else (None, None)
        excl, cand = (csr if kind == "excl" else None), (csr if kind == "cand" else None)
        return ops.knn_score_topk(self.ctx, self._R, self._R_vals, self._W, self._W_vals, start, stop, k, excl=excl, cand=cand)

    def w_csr(self):
        """W as a host scipy CSR."""
        n = self._W.n_rows
        return sp.csr_matrix((self._W_vals[:self._W.nnz].cpu().numpy(), self._W.indices[:self._W.nnz].cpu().numpy(),
                              self._W.indptr.cpu().numpy()), shape=(n, n))

    def get_model_state(self):
        W = self.w_csr()
        return {"_W_data": W.data, "_W_indices": W.indices, "_W_indptr": W.indptr, "_neighborhood": self._neighborhood,
                "_alpha": self._alpha, "_beta": self._beta, "_normalize_similarity": self._normalize_similarity}

    def set_model_state(self, saving_dict):
        self._neighborhood = int(saving_dict["_neighborhood"])
        self._alpha, self._beta = float(saving_dict["_alpha"]), float(saving_dict["_beta"])
        self._normalize_similarity = bool(saving_dict["_normalize_similarity"])
        self._upload_ratings()
        ip = np.asarray(saving_dict["_W_indptr"], np.int64)
        self._W = ops.DeviceCSR(ip, saving_dict["_W_indices"], ip.shape[0] - 1, self.ctx.device)
        self._W_vals = ops.device_values(saving_dict["_W_data"], self.ctx.device)

    def load_weights(self, path):
        with open(path, "rb") as f:
            self.set_model_state(pickle.load(f))

    def save_weights(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.get_model_state(), f)
