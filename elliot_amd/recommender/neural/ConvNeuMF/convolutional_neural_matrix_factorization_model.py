"""ConvNeuralMatrixFactorizationModel on the MI355X -- counterpart of
elliot/recommender/neural/ConvNeuMF/convolutional_neural_matrix_factorization_model.py.

The two embedding tables, the conv tower, the two Dense layers and one Keras Adam live in HBM (ops.ConvNeuMfDeviceState); every numeric
step is a kernel of libelliot_hip.so (el_cnmf.hip).  The reference materialises the [pairs, F, F, 1] interaction maps and
every feature map of a batch, and in get_recs those of a whole chunk of users against all items; here the first feature map is never
stored and a pair leaves one float behind.

Ported as written: `l_b` is read and reaches no loss; the two Dense layers are linear with nothing between them; Keras Adam moves every
row of the two tables every step.  Read from TF 2.3, not run -- parity unpinned vs TF.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel, glorot_uniform


def initial_weights(seed, num_users, num_items, embedding_size, channels, kernels):
    """tf.initializers.GlorotUniform everywhere (biases zero) from a numpy RandomState.  TF's seeded bit stream cannot be reproduced
    without TF -- the distribution is."""
    rs = np.random.RandomState(int(seed))
    w = {"P": glorot_uniform(rs, num_users, embedding_size), "Q": glorot_uniform(rs, num_items, embedding_size), "conv": [], "dense": []}
    for k, cin, cout in zip(kernels, channels[:-1], channels[1:]):
        lim = np.sqrt(6.0 / (k * k * cin + k * k * cout))                      # fan_in, fan_out = receptive field x channels
        w["conv"].append((rs.uniform(-lim, lim, (k, k, cin, cout)).astype(np.float32), np.zeros(cout, np.float32)))
    c = channels[-1]
    w["dense"] = [(glorot_uniform(rs, c, c), np.zeros(c, np.float32)), (glorot_uniform(rs, c, 1), np.zeros(1, np.float32))]
    return w


class ConvNeuralMatrixFactorizationModel(DeviceModel):
    def __init__(self, num_users, num_items, embedding_size, lr, cnn_channels, cnn_kernels, cnn_strides, dropout_prob, l_w, l_b,
                 random_seed=42, name="ConvNeuralMatrixFactorizationModel", ctx=None, init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self._lr, self._l_b = lr, l_b                                            # (l_b: read by the reference, reaches no loss)
        channels, kernels, strides = (list(int(v) for v in x) for x in (cnn_channels, cnn_kernels, cnn_strides))
        if len(kernels) != len(strides) or len(channels) - 1 != len(kernels):
            raise RuntimeError("channels, kernels and strides don't match\n")
        w = init_weights if init_weights is not None else initial_weights(random_seed, num_users, num_items, embedding_size, channels,
                                                                            kernels)
        self.state = ops.ConvNeuMfDeviceState(self.ctx, w, channels, kernels, strides, l_w=l_w, dropout=dropout_prob,
                                              dropout_seed=random_seed)
        self.state.ws_bytes(1, ops._lib.EL_CNMF_WS_FORWARD)                      # a tower outside the supported range is refused here

    def train_step(self, batch):
        """train_step.  batch = (user, pos, neg), shapes [B] or [B, 1]."""
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        self.state.train_step(u, i, j, self._lr)
        return DeferredLoss(self.state)

    def predict(self, inputs, training=False, **kwargs):
        """`call` on (user, item) index arrays of one shape: the prediction alone."""
        user, item = inputs
        shape = tuple(user.shape) if isinstance(user, torch.Tensor) else tuple(np.shape(user))
        return self.state.forward(self._as_index(user), self._as_index(item)).reshape(shape)

    def recommend(self, mask, k, start, stop, item_offset=0):
        """get_recs + get_top_k for the chunk of users [start, stop): el_cnmf_scores on the item image, then el_dense_topk."""
        if not self._items_unchanged():
            self.state.touch()
        return self.state.recommend(start, stop, k, **ops.mask_kwargs(mask))

    # -- checkpoints: the variables in the reference's order, their Adam slots and the step counter ---------------------------
    def get_model_state(self):
        d = {"_step": self.state.step}
        for n in self.state.names:
            for pre in ("", "m", "v"):
                d[pre + n] = getattr(self.state, pre + n).cpu().numpy()
        return d

    def set_model_state(self, d):
        self._touch()
        self.state.touch()
        for n in self.state.names:
            for pre in ("", "m", "v"):
                if pre + n in d:
                    t = getattr(self.state, pre + n)
                    t.copy_(torch.from_numpy(np.ascontiguousarray(d[pre + n])).reshape(t.shape))
        self.state.step = int(d.get("_step", 0))
