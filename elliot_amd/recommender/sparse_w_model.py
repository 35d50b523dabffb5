"""Model half shared by the baselines whose model is the train matrix R and a sparse square W (ItemKNN / UserKNN, RP3beta, Slim):
R and W live on the device as CSRs, ops.knn_score_topk scores and selects per block of users without the [U, I] block, and the
checkpoint is W as a host CSR (`_W_data`, `_W_indices`, `_W_indptr`) beside the subclass's hyper-parameters.

A subclass gives initialize() (which builds _W / _W_vals), hyper_state() and set_hyper_state().
"""
import numpy as np
import scipy.sparse as sp

from .. import ops
from .device_model import DeviceModel


class SparseWModel(DeviceModel):

    def __init__(self, data, ctx):
        self._data = data
        self.ctx = ctx
        self._W = self._W_vals = self._R = self._R_vals = None

    def _urm(self):
        return sp.csr_matrix(self._data.sp_i_train_ratings, dtype=np.float32)

    def _upload_ratings(self, R=None):
        """R on the device, rows in their stored order (the order scipy sums A's row in)."""
        R = self._urm() if R is None else R
        self._R = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], self.ctx.device)
        self._R_vals = ops.device_values(R.data, self.ctx.device)

    def _operands(self):
        """(A, A's values, B, B's values) of the scores A . B: R . W."""
        return self._R, self._R_vals, self._W, self._W_vals

    def recommend(self, mask, k, start, stop):
        """Top-k of users [start, stop) under the tagged mask ("excl" | "cand", DeviceCSR): (idx, val) [n, k] on the device."""
        return ops.knn_score_topk(self.ctx, *self._operands(), start, stop, k, **ops.mask_kwargs(mask))

    def w_csr(self):
        """W as a host scipy CSR."""
        n = self._W.n_rows
        return sp.csr_matrix((self._W_vals[:self._W.nnz].cpu().numpy(), self._W.indices[:self._W.nnz].cpu().numpy(),
                              self._W.indptr.cpu().numpy()), shape=(n, n))

    def get_model_state(self):
        W = self.w_csr()
        return {"_W_data": W.data, "_W_indices": W.indices, "_W_indptr": W.indptr, **self.hyper_state()}

    def set_model_state(self, saving_dict):
        self.set_hyper_state(saving_dict)
        self._upload_ratings()
        ip = np.asarray(saving_dict["_W_indptr"], np.int64)
        self._W = ops.DeviceCSR(ip, saving_dict["_W_indices"], ip.shape[0] - 1, self.ctx.device)
        self._W_vals = ops.device_values(saving_dict["_W_data"], self.ctx.device)
