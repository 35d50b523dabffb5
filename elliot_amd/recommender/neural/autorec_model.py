"""What UserAutoRecModel and ItemAutoRecModel share on the MI355X -- counterpart of
elliot/recommender/neural/UserAutoRec/userautorec_model.py:54-123 and .../ItemAutoRec/itemautorec_model.py:51-131.

    h = sigmoid(x W1 + b1);  r = act(h W2 + b2);  loss = mean_b sum_j ((x - r sign(x))_bj)^2

`x` is a block of rows of a binary matrix: users x items for the user variant (linear head), items x users for the item variant
(sigmoid head).  A batch is the int32 row ids on the device; the step evaluates the decoder at the batch's entries only
(el_autorec_train_step), which is all the loss reads.  `l_w` is accepted and ignored exactly like the reference: its
kernel_regularizers are never added to the loss (train_step uses the squared error alone, :93-107 / :90-104).
"""
import numpy as np
import torch

from ... import ops
from ..autoencoders.vae.multi_vae_model import _glorot_normal
from ..device_model import DeferredLoss, DeviceModel

WEIGHT_ORDER = ("W1", "b1", "W2", "b2")          # keras.Model.get_weights(): encoder kernel, bias, decoder kernel, bias


class AutoRecModel(DeviceModel):
    out_act = None                               # "sigmoid" in the item variant

    def __init__(self, data, num_users, num_items, lr, hidden_neuron, l_w, random_seed=42, name="AutoRec", ctx=None,
                 train_csr=None, max_batch=512, init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self.data, self.num_users, self.num_items = data, num_users, num_items
        self.lr, self.hidden_neuron, self.l_w = lr, int(hidden_neuron), l_w
        self.train_csr = train_csr               # the rows a batch is drawn from; its columns are the layer width
        N, H = int(train_csr.n_cols), self.hidden_neuron
        if init_weights is None:
            # GlorotNormal kernels, biases of ones (:26-30, :39-46); TF's bit stream is not reproducible without TF
            rs = np.random.RandomState(random_seed)
            init_weights = {"W1": _glorot_normal(rs, N, H), "b1": np.ones(H, np.float32),
                            "W2": _glorot_normal(rs, H, N), "b2": np.ones(N, np.float32)}
        self._max_batch = int(min(max_batch, train_csr.n_rows))
        self._new_state(init_weights)

    def _new_state(self, weights):
        # the entries of the largest batch: the max_batch longest rows (a batch never repeats a row)
        lens = (self.train_csr.indptr[1:] - self.train_csr.indptr[:-1])
        nnz_max = int(torch.topk(lens, self._max_batch).values.sum().item()) if lens.numel() else 0
        self.state = ops.AutoRecDeviceState(self.ctx, weights, self.out_act, self._max_batch, nnz_max)

    def train_step(self, batch):
        rows = batch if isinstance(batch, torch.Tensor) else torch.as_tensor(np.asarray(batch), dtype=torch.int32)
        rows = rows.to(device=self.ctx.device, dtype=torch.int32).contiguous()
        self.state.train_step(self.train_csr, rows, self.lr)
        return DeferredLoss(self.state)

    def predict_rows(self, rows):
        """predict (:109-119 / :106-116) on rows of the train matrix: [len(rows), N] on the device."""
        return self.state.predict_rows(self.train_csr, rows.to(device=self.ctx.device, dtype=torch.int32).contiguous())

    def _topk(self, preds, mask, k, start, stop):
        return ops.dense_topk(self.ctx, preds, start, stop, k, **ops.mask_kwargs(mask))

    def get_top_k(self, preds, train_mask, k=100, offset=0):                 # the block's first row is `offset`, not user 0
        idx, val = self._topk(preds, train_mask, k, int(offset), int(offset) + preds.shape[0])
        return val, idx

    # -- checkpoints: the reference's weight order, Keras' layouts ------------------------------------------------------------
    def get_model_state(self):
        w = self.state.weights()
        return {"weights": [w[n] for n in WEIGHT_ORDER]}

    def set_model_state(self, saved):
        self._new_state(dict(zip(WEIGHT_ORDER, saved["weights"])))
