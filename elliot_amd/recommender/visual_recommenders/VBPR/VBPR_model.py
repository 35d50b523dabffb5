"""VBPRModel on the MI355X -- counterpart of elliot/recommender/visual_recommenders/VBPR/VBPR_model.py:15-115.

Same constructor arguments plus `features`, the [num_items, num_image_feature] fp32 matrix in private-item order on the device
(the reference is handed the rows inside every batch instead); `train_step(batch)` with batch = (user, pos, neg), scoring through
`recommend(...)` / `rank(...)`, `save_weights` / `load_weights`.  Bi, Gu, Gi, Tu, E, Bp and one Adam live in HBM
(ops.VbprDeviceState); every numeric step is a kernel of libelliot_hip.so (el_vbpr.hip).

Scoring restates predict_item_batch (:104-108) for all items at once: the image ([Gu | Tu], [Gi | F E], Bi + F Bp) is rebuilt when
the weights changed since the last scoring, then el_score_topk / el_score_rank run on it.  `predict` (:98-101) reads an attribute
`self.F` that nothing sets; it cannot run in the reference and is not ported.
"""
import numpy as np
import torch

from .... import ops
from ...device_model import DeferredLoss, DeviceModel, glorot_uniform

NAMES = ("Bi", "Gu", "Gi", "Tu", "E", "Bp")            # the reference's six variables: the keys of a checkpoint


def initial_weights(seed, num_users, num_items, factors, factors_d, num_image_feature):
    """tf.initializers.GlorotUniform for the five matrices, drawn on the host in the order the reference creates its variables
    (:40-51): Bi = 0, then Gu, Gi, Bp, Tu, E.  TF's seeded bit stream cannot be reproduced without TF -- the distribution is
    (SURVEY A.5)."""
    rs = np.random.RandomState(seed)
    w = {"Bi": np.zeros(num_items, np.float32)}
    w["Gu"], w["Gi"] = glorot_uniform(rs, num_users, factors), glorot_uniform(rs, num_items, factors)
    w["Bp"] = glorot_uniform(rs, num_image_feature, 1)
    w["Tu"], w["E"] = glorot_uniform(rs, num_users, factors_d), glorot_uniform(rs, num_image_feature, factors_d)
    return w


class VBPRModel(DeviceModel):
    def __init__(self, factors=200, factors_d=20, learning_rate=0.001, l_w=0, l_b=0, l_e=0, num_image_feature=2048, num_users=100,
                 num_items=100, random_seed=42, name="VBPRMF", ctx=None, features=None, init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self._factors, self._factors_d, self._learning_rate = factors, factors_d, learning_rate
        self._l_w, self._l_b, self._l_e = l_w, l_b, l_e
        self.num_image_feature, self._num_users, self._num_items = num_image_feature, num_users, num_items
        if features is None or tuple(features.shape) != (num_items, num_image_feature):
            raise ValueError(f"VBPRModel: `features` must be the [{num_items}, {num_image_feature}] item feature matrix")
        if init_weights is None:
            init_weights = initial_weights(random_seed, num_users, num_items, factors, factors_d, num_image_feature)
        Bi, Gu, Gi, Tu, E, Bp = (init_weights[n] for n in NAMES)
        self.vb = ops.VbprDeviceState(self.ctx, Gu, Gi, Bi, Tu, E, Bp, features)
        self.state = self.vb.base                                 # (Gu, Gi, Bi, their slots and the step counter)
        self._image_version = -1

    # -- training ---------------------------------------------------------------------------------------
    def train_step(self, batch):
        """train_step (:70-95).  batch = (user, pos, neg), shapes [B] or [B, 1]; the feature rows are looked up on the device."""
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        self.vb.train_step(u, i, j, self._learning_rate, self._l_w, self._l_b, self._l_e)
        return DeferredLoss(self.vb)

    # -- scoring ----------------------------------------------------------------------------------------
    def _image(self):
        """([Gu | Tu], [Gi | F E], Bi + F Bp), rebuilt when the weights changed since it was last built; and whether the item
        side is what the previous scoring call saw."""
        if self._image_version != self._weights_version:
            self._image_version = self._weights_version
            self._scored_version = -1
            self.vb.image()
        return self.vb._P, self.vb._Q, self.vb._bq, self._items_unchanged()

    def recommend(self, mask, k, start, stop, item_offset=0):
        P, Q, bq, same = self._image()
        return ops.score_topk(self.ctx, P, Q, bq, start, stop, k, **ops.mask_kwargs(mask), item_offset=item_offset, items_unchanged=same)

    def rank(self, mask, targets, start, stop):
        P, Q, bq, _ = self._image()
        return ops.score_rank(self.ctx, P, Q, bq, start, stop, targets, **ops.mask_kwargs(mask))

    # -- checkpoints: the reference's six variable names, the Adam slots and the step counter -----------------
    def _tensors(self):
        st, vb = self.state, self.vb
        return {"Bi": (st.Bi, st.mBi, st.vBi), "Gu": (st.Gu, st.mGu, st.vGu), "Gi": (st.Gi, st.mGi, st.vGi),
                "Tu": (vb.Tu, vb.mTu, vb.vTu), "E": (vb.EB[:, :vb.Fd], vb.mEB[:, :vb.Fd], vb.vEB[:, :vb.Fd]),
                "Bp": (vb.EB[:, vb.Fd:], vb.mEB[:, vb.Fd:], vb.vEB[:, vb.Fd:])}

    def get_model_state(self):
        d = {"_step": self.state.step}
        for n, (th, m, v) in self._tensors().items():
            d[n], d["m" + n], d["v" + n] = th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
        return d

    def set_model_state(self, d):
        self._touch()
        for n, (th, m, v) in self._tensors().items():
            th.copy_(torch.from_numpy(np.ascontiguousarray(d[n])).reshape(th.shape))
            for slot, t in (("m" + n, m), ("v" + n, v)):
                if slot in d:
                    t.copy_(torch.from_numpy(np.ascontiguousarray(d[slot])).reshape(t.shape))
        self.state.step = int(d.get("_step", 0))
