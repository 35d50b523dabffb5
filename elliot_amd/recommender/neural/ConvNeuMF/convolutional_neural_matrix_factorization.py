"""ConvNeuMF plugin (YAML key `external.ConvNeuMF`): Outer Product-based Neural Collaborative Filtering (He et al., IJCAI 2018,
https://arxiv.org/abs/1808.03912).

Contract of elliot/recommender/neural/ConvNeuMF/convolutional_neural_matrix_factorization.py: hyper-parameters `lr`, `embedding_size`,
`cnn_channels`, `cnn_kernels`, `cnn_strides`, `dropout_prob`, `l_w`, `l_b` with the same file-name shortcuts, result-file name
"ConvNeuMF_...", the BPR triplet sampler of BPRMF_batch (philox, or `sampler: replay`), an epoch of `step(transactions, batch_size)`,
the epoch loss handed to evaluate() as loss / (it + 1), users scored in chunks of `batch_size`.  The training loop is RecMixin.train().

  cnn_kernels == cnn_strides   only non-overlapping patches are offered (the reference's default and the paper's tower); anything else
                               is refused by the library, which names the option.
  l_b                          accepted and without effect: the reference reads it and it reaches no loss.
"""
from ast import literal_eval as make_tuple

from .... import ops
from ....dataset.samplers import custom_sampler
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from .convolutional_neural_matrix_factorization_model import ConvNeuralMatrixFactorizationModel


class ConvNeuMF(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        units = lambda x: list(make_tuple(str(x)))                                                 # noqa: E731
        show = lambda x: self._batch_remove(str(x), " []").replace(",", "-")                       # noqa: E731
        self._params_list = [
            param("lr", "lr", 0.001),
            param("embedding_size", "embedding_size", 100),
            param("cnn_channels", "cnn_channels", "(1, 32, 32)", read=units, show=show),
            param("cnn_kernels", "cnn_kernels", "(2,2)", read=units, show=show),
            param("cnn_strides", "cnn_strides", "(2,2)", read=units, show=show),
            param("dropout_prob", "dropout_prob", 0),
            param("l_w", "l_w", 0.005),
            param("l_b", "l_b", 0.0005),
        ]
        self.autoset_params()
        if self._batch_size < 1:
            self._batch_size = self._data.transactions
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        replay = getattr(self._params, "sampler", "philox") == "replay"
        positives = self._data.i_train_dict if replay else self._data.sp_i_train
        self._sampler = custom_sampler.Sampler(positives, ctx=self._ctx, replay=replay)
        self._model = ConvNeuralMatrixFactorizationModel(self._num_users, self._num_items, int(self._embedding_size), self._lr,
                                                         self._cnn_channels, self._cnn_kernels, self._cnn_strides, self._dropout_prob,
                                                         self._l_w, self._l_b, self._seed, ctx=self._ctx,
                                                         init_weights=kwargs.get("init_weights"))

    def _recommendation_block(self):
        return int(self._batch_size)

    @property
    def name(self):
        return "ConvNeuMF" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"
