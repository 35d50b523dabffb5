"""UserAutoRec plugin (YAML key `external.UserAutoRec`) -- AutoRec: Autoencoders Meet Collaborative Filtering (user-based),
https://users.cecs.anu.edu.au/~akmenon/papers/autorec/autorec-paper.pdf.

Contract of elliot/recommender/neural/UserAutoRec/userautorec.py:21-98: hyper-parameters `lr` (0.0001), `hidden_neuron` (500),
`l_w` (0.001; it never reaches the reference's loss, so it does nothing here either) + base keys; `batch_size` < 1 means all users
in one batch; the epoch loss is handed to evaluate() as sum / (epoch + 1) (:98).
"""
from tqdm import tqdm

from .... import ops
from ....dataset.samplers import sparse_sampler
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from .userautorec_model import UserAutoRecModel


class UserAutoRec(RecMixin, BaseRecommenderModel):
    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("lr", "lr", 0.0001, attr="_lr"),
            param("hidden_neuron", "hidden_neuron", 500, int),
            param("l_w", "l_w", 0.001),
        ]
        self.autoset_params()
        if self._batch_size < 1:
            self._batch_size = self._num_users
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._sampler = sparse_sampler.Sampler(self._data.sp_i_train, ctx=self._ctx)
        self._score_block = min(max(self._batch_size, 1), 2048)
        self._model = UserAutoRecModel(self._data, self._num_users, self._num_items, self._lr, self._hidden_neuron, self._l_w,
                                       self._seed, ctx=self._ctx, train_csr=self._sampler.train, max_batch=self._batch_size,
                                       init_weights=kwargs.get("init_weights"))

    @property
    def name(self):
        return "_".join(["UserAutoRec", self.get_base_params_shortcut(), self.get_params_shortcut()])

    def _recommendation_block(self):
        return self._score_block                                     # dense [block, I] reconstruction

    def train(self):
        if self._restore:
            return self.restore_weights()
        for it in self.iterate(self._epochs):
            loss = 0
            with tqdm(total=int(self._num_users // self._batch_size), disable=not self._verbose) as bar:
                for batch in self._sampler.step(self._num_users, self._batch_size):
                    loss += self._model.train_step(batch)
                    bar.update()
            self.evaluate(it, float(loss) / (it + 1))
