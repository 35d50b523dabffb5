"""Model half of Slim (slim_model.py: train, prepare_predictions, get_user_recs).

What the reference computes -- one sklearn ElasticNet.fit per item in a Python loop, the cut of every column, the dense
R.dot(W), a masked top-k per user -- is done on the device without the dense score matrix: ops.slim_build (el_slim_order,
el_slim_fit over blocks of target columns, el_slim_w) and ops.knn_score_topk per block of users.
"""
import pickle

import numpy as np
import scipy.sparse as sp

from .... import ops


class SlimModel(object):

    def __init__(self, data, l1_ratio, alpha, neighborhood, random_seed, exclusion, ctx):
        self._data = data
        self._l1_ratio = float(l1_ratio)
        self._alpha = float(alpha)
        self._neighborhood = int(neighborhood)
        self._seed = int(random_seed)
        self._exclusion = str(exclusion)
        self.ctx = ctx
        self._W = self._W_vals = self._R = self._R_vals = None
        self.n_iter = None

    def _urm(self):
        return sp.csr_matrix(self._data.sp_i_train_ratings, dtype=np.float32)

    def _upload_ratings(self):
        """R on the device, rows in their stored order (the order scipy sums A's row in)."""
        R = self._urm()
        self._R = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], self.ctx.device)
        self._R_vals = ops.device_values(R.data, self.ctx.device)

    def initialize(self):
        self._upload_ratings()
        csc, csc_vals = ops.slim_csc(self.ctx, self._urm())
        self._W, self._W_vals, self.n_iter = ops.slim_build(self.ctx, csc, csc_vals, self._alpha, self._l1_ratio, self._neighborhood,
                                                            self._seed, self._exclusion)

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
        return {"_W_data": W.data, "_W_indices": W.indices, "_W_indptr": W.indptr, "_l1_ratio": self._l1_ratio,
                "_alpha": self._alpha, "_neighborhood": self._neighborhood, "_seed": self._seed, "_exclusion": self._exclusion}

    def set_model_state(self, saving_dict):
        self._l1_ratio, self._alpha = float(saving_dict["_l1_ratio"]), float(saving_dict["_alpha"])
        self._neighborhood, self._seed = int(saving_dict["_neighborhood"]), int(saving_dict["_seed"])
        self._exclusion = str(saving_dict["_exclusion"])
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
