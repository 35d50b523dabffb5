"""AMF_model on the MI355X -- counterpart of elliot/recommender/adversarial/AMF/AMF_model.py:17-197.

Same constructor arguments; `train_step(batch, user_adv_train)`, `build_perturbation`, `build_msap_perturbation`, scoring through
`recommend(..., adversarial=)`, `save_weights` / `load_weights`.  Gu, Gi, Bi, one Adam and the two perturbation tables live in HBM
(ops.AmfDeviceState); every numeric step is a kernel of libelliot_hip.so.

The reference's `adversarial` flag reads the other way round from its name: call(adversarial=False) gathers from Gu + Delta_Gu,
Gi + Delta_Gi, call(adversarial=True) from the plain tables (:58-63).  It is ported as written: a step's "clean" loss and its
regulariser read the perturbed rows, the l_adv term reads the plain ones.  While the perturbation is all zero (before the first
adversarial step, or with adversarial_epochs = 0) a plain step IS BPRMF_batch's, and takes its kernels.
"""
import torch

from .... import ops
from ...device_model import DeferredLoss
from ...latent_factor_models.BPRMF_batch.BPRMF_batch_model import BPRMF_batch_model, initial_weights


class AMF_model(BPRMF_batch_model):
    def __init__(self, factors=200, learning_rate=0.001, l_w=0, l_b=0, eps=0, l_adv=0, num_users=100, num_items=100,
                 random_seed=42, name="AMF", ctx=None, init_weights=None, **kwargs):
        self.ctx = ctx or ops.get_context(0)
        self._factors, self._learning_rate, self._l_w, self._l_b = factors, learning_rate, l_w, l_b
        self._eps, self._l_adv = eps, l_adv
        self._num_users, self._num_items = num_users, num_items
        # tf.initializers.GlorotUniform (:40-43) as BPRMF_batch_model draws it on the host; Bi = 0
        Gu, Gi, Bi = init_weights if init_weights is not None else initial_weights(random_seed, num_users, num_items, factors)
        self.amf = ops.AmfDeviceState(self.ctx, Gu, Gi, Bi)
        self.state = self.amf.base                               # what BPRMF_batch_model's scoring and checkpoints read

    # -- training ---------------------------------------------------------------------------------------
    def train_step(self, batch, user_adv_train=False):
        """train_step (:70-105).  batch = (user, pos, neg), shapes [B] or [B, 1]."""
        if not user_adv_train and self.amf.delta_is_zero:
            return super().train_step(batch)                     # Delta = 0: the BPRMF_batch step, bit for bit
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        self.amf.train_step(u, i, j, self._learning_rate, self._l_w, self._l_b, self._l_adv, self._eps, bool(user_adv_train))
        return DeferredLoss(self.amf)

    def train_epoch(self, sampler, events, batch_size):
        """A whole epoch of plain steps from one library call; only while the perturbation is all zero."""
        if not self.amf.delta_is_zero:
            raise ValueError("train_epoch: the fused epoch runs BPRMF_batch's plain steps, and a perturbation is in place")
        return super().train_epoch(sampler, events, batch_size)

    def build_perturbation(self, batch):
        """FGSM (:133-161): Delta = eps * normalize(grad) on the batch's rows, zero elsewhere."""
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        self.amf.perturb(u, i, j, self._l_w, self._l_b, self._eps)

    def build_msap_perturbation(self, batch, eps_iter, nb_iter):
        """MSAP (:163-197): nb_iter clipped steps of size eps_iter."""
        u, i, j = (self._as_index(x) for x in batch)
        self._touch()
        if int(nb_iter) < 1:
            self.amf.clear_delta()                               # (the reference's loop body never runs: Delta stays zero)
            return
        self.amf.perturb(u, i, j, self._l_w, self._l_b, self._eps, eps_iter, int(nb_iter))

    # -- scoring ----------------------------------------------------------------------------------------
    def _tables(self, adversarial):
        st = self.state
        if adversarial:                                          # predict(adversarial=True), :109-111: sums first, then the product
            Pu, Pi = self.amf.perturbed_tables()
            return Pu, Pi, st.Bi
        return st.Gu, st.Gi, st.Bi

    def recommend(self, mask, k, start, stop, item_offset=0, adversarial=False):
        if not adversarial:
            return super().recommend(mask, k, start, stop, item_offset)
        self._scored_version = -1                                # the item image of the screened kernels is another table's now
        Gu, Gi, Bi = self._tables(True)
        return ops.score_topk(self.ctx, Gu, Gi, Bi, start, stop, k, **ops.mask_kwargs(mask), item_offset=item_offset)

    def rank(self, mask, targets, start, stop, adversarial=False):
        Gu, Gi, Bi = self._tables(adversarial)
        return ops.score_rank(self.ctx, Gu, Gi, Bi, start, stop, targets, **ops.mask_kwargs(mask))

    # -- checkpoints: BPRMF_batch's keys plus the perturbation ---------------------------------------------
    def get_model_state(self):
        d = super().get_model_state()
        d["_delta_Gu"], d["_delta_Gi"] = self.amf.dGu.cpu().numpy(), self.amf.dGi.cpu().numpy()
        return d

    def set_model_state(self, d):
        super().set_model_state(d)
        zu, zi = torch.zeros_like(self.amf.dGu), torch.zeros_like(self.amf.dGi)
        self.amf.set_delta(d.get("_delta_Gu", zu), d.get("_delta_Gi", zi))
