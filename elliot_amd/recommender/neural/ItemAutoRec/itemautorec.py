"""ItemAutoRec plugin (YAML key `external.ItemAutoRec`) -- AutoRec: Autoencoders Meet Collaborative Filtering (item-based),
https://users.cecs.anu.edu.au/~akmenon/papers/autorec/autorec-paper.pdf.

Contract of elliot/recommender/neural/ItemAutoRec/itemautorec.py:20-108: hyper-parameters `lr` (0.0001), `hidden_neuron` (500),
`l_w` (0.001; it never reaches the reference's loss, so it does nothing here either) + base keys; the batches are rows of the
TRANSPOSED train matrix (:67-68); `batch_size` < 1 means all items in one batch; the epoch loss is handed to evaluate() as
sum / (epoch + 1) (:97).

`item_order`.  The reference evaluates through `self._sampler.step(num_items, num_items)` (:102), which draws a fresh shuffle: the
columns of the block it ranks are the items in SHUFFLED order, yet column c is reported (and masked) as item c.
  item_order: model       (default) column c is item c -- the model's own ranking
  item_order: reference   column c holds the prediction of the c-th item of that shuffle, as the reference ranks it
Either way one `random.sample` is drawn per evaluation, so the training batches that follow are the reference's.
"""
import random

from tqdm import tqdm

from .... import ops
from ....dataset.samplers import sparse_sampler
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from .itemautorec_model import ItemAutoRecModel


class ItemAutoRec(RecMixin, BaseRecommenderModel):
    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("lr", "lr", 0.0001, attr="_lr"),
            param("hidden_neuron", "hidden_neuron", 500, int),
            param("l_w", "l_w", 0.001),
        ]
        self.autoset_params()
        if self._batch_size < 1:
            self._batch_size = self._num_items
        self._item_order = str(getattr(self._params, "item_order", "model"))
        if self._item_order not in ("model", "reference"):
            raise ValueError(f"item_order must be 'model' or 'reference', got {self._item_order!r}")
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._sampler = sparse_sampler.Sampler(self._data.sp_i_train.transpose(), ctx=self._ctx)        # :67-68
        self._score_block = 2048
        self._model = ItemAutoRecModel(self._data, self._num_users, self._num_items, self._lr, self._hidden_neuron, self._l_w,
                                       self._seed, ctx=self._ctx, train_csr=self._sampler.train, max_batch=self._batch_size,
                                       init_weights=kwargs.get("init_weights"))

    @property
    def name(self):
        return "_".join(["ItemAutoRec", self.get_base_params_shortcut(), self.get_params_shortcut()])

    def _recommendation_block(self):
        return self._score_block                                     # dense [block, I] transposed reconstruction

    def train(self):
        if self._restore:
            return self.restore_weights()
        for it in self.iterate(self._epochs):
            loss = 0
            with tqdm(total=int(self._num_items // self._batch_size), disable=not self._verbose) as bar:
                for batch in self._sampler.step(self._num_items, self._batch_size):
                    loss += self._model.train_step(batch)
                    bar.update()
            self.evaluate(it, float(loss) / (it + 1))

    def _draw_eval_order(self):
        shuffled = random.sample(range(self._num_items), self._num_items)          # sparse_sampler.py:21 through itemautorec.py:102
        self._model.set_eval_order(shuffled if self._item_order == "reference" else None)

    def get_recommendations(self, k: int = 100):
        self._draw_eval_order()
        return super().get_recommendations(k)

    def _evaluate_on_device(self, k):
        self._draw_eval_order()
        return super()._evaluate_on_device(k)
