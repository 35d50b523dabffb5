"""BPRSlim plugin (YAML key `BPRSlim` / `external.BPRSlim`) -- SLIM (Ning & Karypis 2011) trained with the BPR criterion of
Rendle et al. 2009: a dense item-item matrix S, x_ui = sum of S[i, s] over the items s the user has seen.

Contract of elliot/recommender/latent_factor_models/BPRSlim/bprslim.py: hyper-parameters `lr` (0.001), `lj_reg` (0.001),
`li_reg` (0.1) with the reference's shortcuts and name; `batch_size` below 1 means the number of transactions; an epoch draws
`transactions` triplets and hands evaluate() the sum of their losses x_uij ** 2 over (epoch + 1); checkpoints are the
reference's pickle of {'_s_dense': S} and load in both directions.  Extra optional keys: `sampler` (philox | replay) and `gpu`.

    models:
      BPRSlim:
        meta: {save_recs: True}
        epochs: 10
        batch_size: 512
        lr: 0.001
        lj_reg: 0.001
        li_reg: 0.1

Deviations, all documented:
  * the model is one triplet after the other in sampler order for EVERY `batch_size`.  The reference's train_step takes the
    sampler's [B, 1] arrays as scalars: it runs with `batch_size: 1` only and raises a ValueError for any larger batch.  Here the
    batch size names the run and cannot change the result: an epoch is one sampler call and one level schedule;
  * S starts from zero (the reference starts it from np.empty);
  * a triplet's sum over the seen items is taken in a fixed tree, not left to right, so a trained S follows the reference's
    within the reference's own sensitivity to that order; given S, every prediction is the reference's bit for bit;
  * equal predictions are listed by ascending item index, where the reference's argpartition leaves an arbitrary order;
  * masked items never fill a short list: it is padded with (-1, -inf) and the padding is dropped from the dicts;
  * the device memory S, the scoring table and one score block need is checked before anything is allocated; too little is
    refused with a ValueError stating the bytes.
"""
from .... import ops
from ....dataset.samplers import custom_sampler
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .bprslim_model import BPRSlimModel


class BPRSlim(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (bprslim.py:55-59)
        self._params_list = [
            ("_lr", "lr", "lr", 0.001, None, None),
            ("_lj_reg", "lj_reg", "ljreg", 0.001, None, None),
            ("_li_reg", "li_reg", "lireg", 0.1, None, None),
        ]
        self.autoset_params()
        if self._batch_size < 1:
            self._batch_size = self._data.transactions
        self._ratings = self._data.train_dict
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = BPRSlimModel(self._data, self._lr, self._lj_reg, self._li_reg, self._ctx)
        kind = getattr(self._params, "sampler", "philox")
        if kind not in ("philox", "replay"):
            raise ValueError(f"sampler {kind!r} is not supported; supported: ['philox', 'replay']")
        if kind == "replay":
            self._sampler = custom_sampler.Sampler(self._data.i_train_dict, ctx=self._ctx, replay=True)
        else:
            self._sampler = custom_sampler.Sampler(self._data.sp_i_train, ctx=self._ctx)

    @property
    def name(self):
        return "BPRSlim" \
               + f"_{self.get_base_params_shortcut()}" \
               + f"_{self.get_params_shortcut()}"

    def train(self):
        if self._restore:
            return self.restore_weights()
        n = self._data.transactions
        for it in self.iterate(self._epochs):
            loss = 0
            # the reference walks the epoch one triplet after the other; one sampler call and one level schedule over the whole
            # epoch apply the same sequence, whatever the batch size
            for epoch_triplets in self._sampler.step(n, n):
                loss += self._model.train_step(epoch_triplets)
            self.evaluate(it, loss / (it + 1))
