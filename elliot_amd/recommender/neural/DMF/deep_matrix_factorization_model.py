"""DeepMatrixFactorizationModel on the MI355X -- counterpart of elliot/recommender/neural/DMF/deep_matrix_factorization_model.py.

The two MLPs and one Keras Adam live in HBM (ops.DmfDeviceState); every numeric step is a kernel of libelliot_hip.so (el_dmf.hip,
DESIGN 3.32).  The reference holds two dense [U, I] / [I, U] float "embeddings" and gathers [users, I, I] in get_recs; here the
rating matrix stays CSR with values, a step touches the batch's distinct rows once, and a chunk's scores are one product Pt Qt^T.

Ported as written: `cosine` normalises along the BATCH axis (`cosine_axis: reference`; `row` is the paper's cosine),
in get_recs too, where the scores therefore depend on the chunking; `reg` is read and reaches no loss; Keras Adam moves every element
of every kernel every step.  Read from TF 2.3, not run -- parity unpinned vs TF.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel


def initial_weights(seed, num_users, num_items, user_mlp, item_mlp):
    """Dense kernels RandomNormal(stddev=0.01) (:44), biases zero, drawn from the seeded torch generator.  TF's seeded bit stream cannot
    be reproduced without TF -- the distribution is."""
    gen = torch.Generator().manual_seed(int(seed))
    out = {}
    for side, first, units in (("user", num_items, user_mlp), ("item", num_users, item_mlp)):
        widths = [int(first)] + [int(x) for x in units]
        out[side] = [((torch.randn(a, b, generator=gen, dtype=torch.float64) * 0.01).float().numpy(), np.zeros(b, np.float32))
                     for a, b in zip(widths[:-1], widths[1:])]
    return out


class DeepMatrixFactorizationModel(DeviceModel):
    def __init__(self, num_users, num_items, user_mlp, item_mlp, reg, similarity, max_ratings, sp_i_train_ratings, learning_rate=0.01,
                 random_seed=42, name="DMF", ctx=None, cosine_axis="reference", init_weights=None, **kwargs):
        if similarity not in ("cosine", "dot"):
            raise NotImplementedError(f"DMF: similarity {similarity!r} (cosine | dot)")
        self.ctx = ctx or ops.get_context(0)
        self._lr, self._reg = learning_rate, reg                                        # (reg: read by the reference, reaches no loss)
        w = init_weights if init_weights is not None else initial_weights(random_seed, num_users, num_items, user_mlp, item_mlp)
        R = sp_i_train_ratings.tocsr()
        self.state = ops.DmfDeviceState(self.ctx, w, (R.indptr, R.indices, R.data), similarity=similarity, cosine_axis=cosine_axis,
                                        max_rating=float(max_ratings))

    def _touch(self):
        super()._touch()
        self.state.touch()

    def train_step(self, batch):
        """train_step (:94-105).  batch = (user, item, label), shapes [B] or [B, 1]."""
        user, item, label = batch
        y = label if isinstance(label, torch.Tensor) else torch.from_numpy(np.asarray(label, dtype=np.float32))
        y = y.reshape(-1).to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._touch()
        self.state.train_step(self._as_index(user), self._as_index(item), y, self._lr)
        return DeferredLoss(self.state)

    def predict(self, inputs, training=False, **kwargs):
        """`call` (:84-91) on (user, item) index arrays of one shape, taken as one batch."""
        user, item = inputs
        shape = tuple(user.shape) if isinstance(user, torch.Tensor) else tuple(np.shape(user))
        return self.state.forward(self._as_index(user), self._as_index(item)).reshape(shape)

    def recommend(self, mask, k, start, stop, item_offset=0):
        """get_recs + get_top_k for the chunk of users [start, stop): el_dmf_scores, then el_dense_topk."""
        return self.state.recommend(start, stop, k, **ops.mask_kwargs(mask))

    # -- checkpoints: every kernel and bias, their Adam slots and the step counter ------------------------------
    def get_model_state(self):
        d = {"_step": self.state.step}
        for n in self.state.names:
            for pre in ("", "m", "v"):
                d[n[0] + pre + n[1:]] = getattr(self.state, n[0] + pre + n[1:]).cpu().numpy()
        return d

    def set_model_state(self, d):
        self._touch()
        for n in self.state.names:
            for pre in ("", "m", "v"):
                key = n[0] + pre + n[1:]
                if key in d:
                    t = getattr(self.state, key)
                    t.copy_(torch.from_numpy(np.ascontiguousarray(d[key])).reshape(t.shape))
        self.state.step = int(d.get("_step", 0))
