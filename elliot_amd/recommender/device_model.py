"""What the device model classes share: the protocol between a plugin and the states of ops.py that does not depend on the model --
index batches, the version of the weights a scoring call saw, top-k of a dense block, checkpoints as one pickle."""
import pickle

import numpy as np
import torch

from .. import ops


class DeferredLoss:
    """What train_step returns: the batch losses accumulate in a device double; reading the value (float(),
    .numpy(), formatting) synchronises once -- the reference pays a D2H `.numpy()` every step (BPRMF_batch.py:106)."""

    def __init__(self, state):
        self._state = state

    def __add__(self, other):
        return self

    __radd__ = __add__

    def __float__(self):
        return self._state.pop_loss()

    def numpy(self):
        return np.float32(float(self))


def glorot_uniform(rs, rows, cols):
    """tf.initializers.GlorotUniform from a numpy RandomState: U(-L, L), L = sqrt(6 / (rows + cols)), float32 [rows, cols].
    TF's seeded bit stream cannot be reproduced without TF -- the distribution is."""
    lim = np.sqrt(6.0 / (rows + cols))
    return rs.uniform(-lim, lim, size=(rows, cols)).astype(np.float32)


class DeviceModel:
    """A model whose parameters live in a state of ops.py.  A subclass sets `ctx` and gives get_model_state() / set_model_state()."""

    _weights_version, _scored_version = 0, -1

    def _as_index(self, x):
        """A batch column ([B] or [B, 1]; array, list or tensor) as contiguous int32 [B] on the device."""
        if isinstance(x, torch.Tensor):
            return x.reshape(-1).to(device=self.ctx.device, dtype=torch.int32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)).to(self.ctx.device)

    def _touch(self):
        """The weights changed: the next scoring call re-derives what it keeps of the item side."""
        self._weights_version += 1

    def _items_unchanged(self):
        """Whether the previous scoring call saw these weights (block after block of one evaluation); this call has, from here on."""
        same = self._scored_version == self._weights_version
        self._scored_version = self._weights_version
        return same

    def get_top_k(self, predictions, train_mask, k=100):
        """Masked top-k of a materialised [n, I] block of the first n users (compatibility path): (val, idx)."""
        idx, val = ops.dense_topk(self.ctx, predictions, 0, predictions.shape[0], k, **ops.mask_kwargs(train_mask))
        return val, idx

    def save_weights(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.get_model_state(), f)

    def load_weights(self, path):
        with open(path, "rb") as f:
            self.set_model_state(pickle.load(f))
