"""Model half of PureSVD (pure_svd_model.py: train_step, predict, get_user_recs, the checkpoint).

What the reference computes -- one call of sklearn's randomized_svd on the binary float32 train matrix, user_vec = U,
item_vec = (diag(sigma) Vt)^T, a dense user_vec[u] @ item_vec.T and a masked argpartition per user -- is done on the device:
ops.PureSvdDeviceState (el_spmm_csr_f64, el_psvd_orth, el_gram_f64, el_psvd_project, el_psvd_signs; el_score_topk +
el_topk_pad per block of users).  The tables stay on the device between build and top-k.
"""
import numpy as np

from .... import ops
from ...device_model import DeviceModel


class PureSVDModel(DeviceModel):

    def __init__(self, factors, data, random_seed, ctx):
        self._data = data
        self.factors = factors
        self.random_seed = random_seed
        self.ctx = ctx
        self.state = ops.PureSvdDeviceState(ctx, data.sp_i_train, factors, random_seed)
        self._host_tables = None

    def train_step(self):
        self.state.build()
        self._host_tables = None

    def recommend(self, mask, k, start, stop):
        """Top-k of users [start, stop) under the tagged mask ("excl" | "cand", DeviceCSR): (idx, val) [n, k] on the device."""
        return self.state.recommend(mask, k, start, stop)

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by."""
        return self.state.rank(mask, targets, start, stop)

    def _tables(self):
        if self._host_tables is None:
            self._host_tables = (self.state.user_vec.cpu().numpy(), self.state.item_vec.cpu().numpy())
        return self._host_tables

    def predict(self, user, item):
        """The score of one public (user, item) pair: the float32 dot product of their rows (host copies of the tables)."""
        users, items = self._tables()
        u, i = self._data.public_users[user], self._data.public_items[item]
        return np.dot(users[u], items[i])

    def get_model_state(self):
        user_vec, item_vec = self._tables()
        return {"user_vec": user_vec, "item_vec": item_vec}

    def set_model_state(self, saving_dict):
        self.state.set_weights(np.asarray(saving_dict["user_vec"]), np.asarray(saving_dict["item_vec"]))
        self._host_tables = None
