"""LightGCNModel on the MI355X -- counterpart of elliot/recommender/graph_based/lightgcn/LightGCN_model.py:19-172.

Same constructor arguments.  `train_step(batch)` = `_propagate_embeddings` (:68-94, assigned to the variables) + the bias-free BPR
head with the doubled L2 term (:136-167) + Keras Adam; scoring through `recommend(...)` (predict :131-133 + get_top_k :171-172 fused).
The tables start at ZERO, as the reference's `_create_weights` (:63-65) creates them -- where every gradient of the head vanishes and
the model never moves; `init_weights=(Gu, Gi)` injects tables (tests, warm starts).  `n_fold` (:47, :96-109) only cuts TensorFlow's
sparse product into row blocks: accepted and ignored.

Deviation from the reference: `embed_k` (the plugin's `latent_dim`, shortcut `factors`) must be a multiple of 4 -- the propagation kernels move rows as
16-byte vectors -- and the constructor refuses any other width with a ValueError; the reference accepts any width.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel


ADAM_MOMENTS = ("mGu", "vGu", "mGi", "vGi")


def require_multiple_of_4(name, value):
    """The graph kernels' row width: refused here, by parameter name, before anything reaches the device."""
    if int(value) < 4 or int(value) % 4:
        raise ValueError(f"{name}={value}: the graph propagation kernels need a multiple of 4 (rows move as 16-byte vectors)")


def restore_adam(b, d, complete):
    """The Adam state of the tables (a BprmfDeviceState) from a saved dict.  A dict without the moments (an older file) restarts
    Adam as a whole -- step 0 on zero moments -- so that a restored step count never meets moments it does not belong to."""
    b.step = int(d.get("_step", 0)) if complete else 0
    for n in ADAM_MOMENTS:
        if complete:
            getattr(b, n).copy_(torch.from_numpy(d[n]))
        else:
            getattr(b, n).zero_()


class LightGCNModel(DeviceModel):
    def __init__(self, num_users, num_items, learning_rate, embed_k, l_w, n_layers, n_fold, adjacency, laplacian, random_seed,
                 name="LightGCN", ctx=None, init_weights=None, **kwargs):
        require_multiple_of_4("embed_k (latent_dim, factors)", embed_k)
        self.ctx = ctx or ops.get_context(0)
        self.num_users, self.num_items, self.embed_k = int(num_users), int(num_items), int(embed_k)
        self.learning_rate, self.l_w, self.n_layers, self.n_fold = learning_rate, l_w, int(n_layers), n_fold
        if init_weights is not None:
            Gu, Gi = init_weights
        else:
            Gu = np.zeros((self.num_users, self.embed_k), np.float32)          # :64-65 tf.zeros
            Gi = np.zeros((self.num_items, self.embed_k), np.float32)
        lap = laplacian.tocsr()
        lap.sort_indices()
        self.graph = ops.GraphCSR(self.ctx, lap.indptr, lap.indices, lap.data.astype(np.float32), self.num_users, self.embed_k)
        self.state = ops.LightGcnDeviceState(self.ctx, Gu, Gi, self.graph, n_layers=self.n_layers)

    def train_step(self, batch):
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        self.state.train_step(u, i, j, self.learning_rate, self.l_w)
        return DeferredLoss(self.state)

    def recommend(self, mask, k, start, stop, item_offset=0):
        st = self.state
        return ops.score_topk(self.ctx, st.Gu, st.Gi, None, start, stop, k, **ops.mask_kwargs(mask), item_offset=item_offset,
                              items_unchanged=self._items_unchanged())

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by (el_score_rank)."""
        st = self.state
        return ops.score_rank(self.ctx, st.Gu, st.Gi, None, start, stop, targets, **ops.mask_kwargs(mask))

    def get_model_state(self):
        b = self.state.bpr
        b.sync()
        d = {"Gu": b.Gu.cpu().numpy(), "Gi": b.Gi.cpu().numpy(), "_step": b.step}
        for n in ADAM_MOMENTS:
            d[n] = getattr(b, n).cpu().numpy()
        return d

    def set_model_state(self, d):
        b = self.state.bpr
        self._touch()
        b.Gu.copy_(torch.from_numpy(d["Gu"]))
        b.Gi.copy_(torch.from_numpy(d["Gi"]))
        restore_adam(b, d, all(n in d for n in ADAM_MOMENTS))
