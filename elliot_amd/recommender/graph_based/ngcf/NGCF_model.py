"""NGCFModel on the MI355X -- counterpart of elliot/recommender/graph_based/ngcf/NGCF_model.py:18-226.

Same constructor arguments.  `train_step(batch)` = `_propagate_embeddings` (:106-142: sparse product, the two dense transforms, leaky_relu,
message dropout, row normalisation, concat, assigned to the variables) + the bias-free BPR head on the full-width rows with the doubled L2
term (:187-217) + Adam (tables: every-row sparse apply; GraphLayers: their L2-only gradient).  The tables start at ZERO as the reference
creates them (:88-91) -- a state in which the layer-0 columns never receive a gradient -- unless `init_weights=(Gu, Gi[, layers])`
injects them; the GraphLayers follow GlorotUniform ([kin, kout] and [1, kout] limits, :95-104; TensorFlow's seeded stream itself is not
reproducible).  node_dropout (:56-60, :153-158): one fixed sparsification of the Laplacian at construction, keep probability
node_dropout[0], kept entries scaled by 1 / keep.  `n_fold` only cuts TensorFlow's sparse product into row blocks: ignored.

Deviation from the reference: `embed_k` (the plugin's `latent_dim`, shortcut `factors`) and every entry of `weight_size` must be multiples of 4 -- the
propagation kernels move rows as 16-byte vectors -- and the constructor refuses any other width with a ValueError; the reference accepts
any width.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel, glorot_uniform
from ..lightgcn.LightGCN_model import ADAM_MOMENTS, require_multiple_of_4, restore_adam


class NGCFModel(DeviceModel):
    def __init__(self, num_users, num_items, learning_rate, embed_k, l_w, weight_size, n_layers, node_dropout, message_dropout, n_fold,
                 adjacency, laplacian, random_seed, name="NGFC", ctx=None, init_weights=None, **kwargs):
        require_multiple_of_4("embed_k (latent_dim, factors)", embed_k)
        for w in weight_size:
            require_multiple_of_4("weight_size entry", w)
        self.ctx = ctx or ops.get_context(0)
        self.num_users, self.num_items, self.embed_k = int(num_users), int(num_items), int(embed_k)
        self.learning_rate, self.l_w = learning_rate, l_w
        self.weight_size_list = [self.embed_k] + [int(w) for w in weight_size]
        W = sum(self.weight_size_list)
        rs = np.random.RandomState(random_seed)
        layers = None
        if init_weights is not None:
            Gu, Gi = init_weights[0], init_weights[1]
            layers = init_weights[2] if len(init_weights) > 2 else None
        else:
            Gu, Gi = np.zeros((self.num_users, W), np.float32), np.zeros((self.num_items, W), np.float32)     # :88-91 tf.zeros
        if layers is None:
            glorot = lambda a, b: glorot_uniform(rs, a, b)
            layers = []
            for k in range(int(n_layers)):
                kin, kout = self.weight_size_list[k], self.weight_size_list[k + 1]
                layers.append({"W1": glorot(kin, kout), "b1": glorot(1, kout), "W2": glorot(kin, kout), "b2": glorot(1, kout)})
        lap = laplacian.tocsr().astype(np.float32)
        lap.sort_indices()
        vals = lap.data.copy()
        if len(node_dropout):
            keep = float(node_dropout[0])
            mask = np.floor(keep + rs.uniform(size=vals.shape[0])).astype(bool)                                 # :74-83
            vals = np.where(mask, vals * np.float32(1.0 / keep), np.float32(0.0)).astype(np.float32)
        self.graph = ops.GraphCSR(self.ctx, lap.indptr, lap.indices, vals, self.num_users, max(self.weight_size_list))
        drop = [float(x) for x in message_dropout] if len(message_dropout) else [0.0] * int(n_layers)
        self.state = ops.NgcfDeviceState(self.ctx, Gu, Gi, self.graph, layers, self.embed_k, message_dropout=drop, dropout_seed=random_seed)

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
        st, b = self.state, self.state.bpr
        b.sync()
        d = {"Gu": b.Gu.cpu().numpy(), "Gi": b.Gi.cpu().numpy(), "_step": b.step,
             "layers": [{k: v.cpu().numpy() for k, v in l.items()} for l in st.layers],
             "layer_slots": [{k: (m.cpu().numpy(), v.cpu().numpy()) for k, (m, v) in sl.items()} for sl in st.slots]}
        for n in ADAM_MOMENTS:
            d[n] = getattr(b, n).cpu().numpy()
        return d

    def set_model_state(self, d):
        st, b = self.state, self.state.bpr
        self._touch()
        b.Gu.copy_(torch.from_numpy(d["Gu"]))
        b.Gi.copy_(torch.from_numpy(d["Gi"]))
        for l, src in zip(st.layers, d.get("layers", [])):
            for k, v in src.items():
                l[k].copy_(torch.from_numpy(v))
        # the tables' moments, the GraphLayers' (m, v) slots and the step count (which also seeds the message-dropout mask) go together
        complete = all(n in d for n in ADAM_MOMENTS) and "layer_slots" in d
        restore_adam(b, d, complete)
        for sl, src in zip(st.slots, d["layer_slots"] if complete else [{}] * len(st.slots)):
            for k, (m, v) in sl.items():
                if complete:
                    m.copy_(torch.from_numpy(src[k][0])), v.copy_(torch.from_numpy(src[k][1]))
                else:
                    m.zero_(), v.zero_()
