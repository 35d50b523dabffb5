"""BPRMF_batch_model on the MI355X -- counterpart of
elliot/recommender/latent_factor_models/BPRMF_batch/BPRMF_batch_model.py:18-88.

Same constructor arguments; `train_step(batch)`, `predict`-free scoring through `recommend(...)`,
`get_top_k`, `save_weights` / `load_weights`.  Parameters live in HBM (ops.BprmfDeviceState); every numeric
step is a kernel of libelliot_hip.so.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel, glorot_uniform


def initial_weights(seed, num_users, num_items, factors):
    """tf.initializers.GlorotUniform (:39-42) drawn on the host: Gu, then Gi; Bi = 0."""
    rs = np.random.RandomState(seed)
    return glorot_uniform(rs, num_users, factors), glorot_uniform(rs, num_items, factors), np.zeros(num_items, np.float32)


class BPRMF_batch_model(DeviceModel):
    def __init__(self, factors=200, learning_rate=0.001, l_w=0, l_b=0, num_users=100, num_items=100, random_seed=42,
                 name="NNBPRMF", ctx=None, optimizer="adam", init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self._factors, self._learning_rate, self._l_w, self._l_b = factors, learning_rate, l_w, l_b
        self._num_users, self._num_items = num_users, num_items
        if init_weights is not None:
            Gu, Gi, Bi = init_weights
        elif (num_users + num_items) * factors * 4 >= ops.BIG_TABLE_BYTES and kwargs.get("init", "auto") != "host":
            # large tables (a 1 M x 128 user table is 512 MB): the same distribution drawn in HBM -- a host draw + H2D copy of
            # 10^8 floats costs seconds per model instance (one per HPO trial and fold, model_coordinator.py:58-65)
            g = torch.Generator(device=self.ctx.device)
            g.manual_seed(int(random_seed))
            lu, li = (6.0 / (num_users + factors)) ** 0.5, (6.0 / (num_items + factors)) ** 0.5
            Gu = (torch.rand((num_users, factors), generator=g, device=self.ctx.device) * 2 - 1) * lu
            Gi = (torch.rand((num_items, factors), generator=g, device=self.ctx.device) * 2 - 1) * li
            Bi = torch.zeros(num_items, device=self.ctx.device)
        else:
            Gu, Gi, Bi = initial_weights(random_seed, num_users, num_items, factors)
        self.state = ops.BprmfDeviceState(self.ctx, Gu, Gi, Bi, optimizer=optimizer)

    # -- training ---------------------------------------------------------------------------------------
    def train_step(self, batch):
        """BPRMF_batch_model.train_step (:58-80).  batch = (user, pos, neg), shapes [B] or [B, 1]."""
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        self.state.train_step(u, i, j, self._learning_rate, self._l_w, self._l_b)
        return DeferredLoss(self.state)

    def train_epoch(self, sampler, events, batch_size):
        """The whole `for batch in sampler.step(events, batch_size): train_step(batch)` loop of BPRMF_batch.train
        (:100-109) in one library call (el_bprmf_train_loop); same triplets, same updates."""
        first = sampler.advance(events)
        self._touch()
        self.state.train_loop(sampler.pos, events, batch_size, sampler.seed, first, self._learning_rate, self._l_w, self._l_b)
        return DeferredLoss(self.state)

    # -- scoring ----------------------------------------------------------------------------------------
    def recommend(self, mask, k, start, stop, item_offset=0):
        """predict (:83-84) + get_top_k (:87-88) fused: top-k of users [start, stop) under `mask`
        (("excl", csr) | ("cand", csr) | None) -> (idx int32 [n, k], val fp32 [n, k]) device tensors."""
        st = self.state
        return ops.score_topk(self.ctx, st.Gu, st.Gi, st.Bi, start, stop, k, **ops.mask_kwargs(mask), item_offset=item_offset,
                              items_unchanged=self._items_unchanged())

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` (device CSR) in the users' full rankings, in the order
        recommend() selects by (el_score_rank): int32 on the device."""
        st = self.state
        return ops.score_rank(self.ctx, st.Gu, st.Gi, st.Bi, start, stop, targets, **ops.mask_kwargs(mask))

    # -- checkpoints (same keys as the NumPy model's pickle, BPRMF_model.py:119-139, plus optimiser slots) ----
    def get_model_state(self):
        st = self.state
        st.sync()                     # deferred decay: every row of both tables AND of their Adam slots current before anything is read
        d = {"_user_factors": st.Gu.cpu().numpy(), "_item_factors": st.Gi.cpu().numpy(),
             "_item_bias": st.Bi.cpu().numpy(), "_step": st.step}
        for n in ("mGu", "vGu", "mGi", "vGi", "mBi", "vBi"):
            t = getattr(st, n)
            if t is not None:
                d[n] = t.cpu().numpy()
        return d

    def set_model_state(self, d):
        st = self.state
        self._touch()
        st.Gu.copy_(torch.from_numpy(d["_user_factors"]))
        st.Gi.copy_(torch.from_numpy(d["_item_factors"]))
        st.Bi.copy_(torch.from_numpy(d["_item_bias"]))
        st.step = int(d.get("_step", 0))
        for n in ("mGu", "vGu", "mGi", "vGi", "mBi", "vBi"):
            if n in d and getattr(st, n) is not None:
                getattr(st, n).copy_(torch.from_numpy(d[n]))
