"""VBPR plugin (YAML key `external.VBPR`): Visual Bayesian Personalized Ranking (He & McAuley,
http://www.aaai.org/ocs/index.php/AAAI/AAAI16/paper/view/11914).

Contract of elliot/recommender/visual_recommenders/VBPR/VBPR.py:22-144: hyper-parameters `batch_eval`, `factors`, `factors_d`, `lr`,
`l_w`, `l_b`, `l_e`, `loader` (the side-information namespace, default "VisualAttributes"), result-file name "VBPR_...".  The
sampler is BPRMF_batch's (philox, or `sampler: replay` for the reference's MT19937 stream: its sample() draws the same three
integers in the same order); the reference's tf.data pipeline batches ONE stream that runs on across epochs, so an epoch is
`transactions // batch_size` full batches and no batch is ever short (pairwise_pipeline_sampler_vbpr.py:47-70, VBPR.py:115-127).
The item features are not fed with the batches: the loader's matrix, in private-item order, is on the device once.
`batch_eval` is accepted for the file name; scoring needs no item blocks (the image of all items is one small product).
The training loop is RecMixin.train().
"""
from .... import ops
from ....dataset.samplers import custom_sampler
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .VBPR_model import VBPRModel


class VBPR(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            ("_batch_eval", "batch_eval", "be", 512, int, None),
            ("_factors", "factors", "factors", 100, None, None),
            ("_factors_d", "factors_d", "factors_d", 20, None, None),
            ("_learning_rate", "lr", "lr", 0.0005, None, None),
            ("_l_w", "l_w", "l_w", 0.000025, None, None),
            ("_l_b", "l_b", "l_b", 0, None, None),
            ("_l_e", "l_e", "l_e", 0.002, None, None),
            ("_loader", "loader", "load", "VisualAttributes", None, None),
        ]
        self.autoset_params()
        if self._batch_size < 1:
            self._batch_size = self._data.transactions
        if self._batch_size > self._data.transactions:
            raise Exception(f"VBPR: batch_size ({self._batch_size}) is larger than the number of training interactions "
                            f"({self._data.transactions}): an epoch of transactions // batch_size full batches would be empty")
        self._side = getattr(self._data.side_information, self._loader, None)
        if self._side is None or not hasattr(self._side, "feature_matrix"):
            raise Exception(f"VBPR needs the side information `{self._loader}` (dataloader: VisualAttribute with `visual_features`)")
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        items = [self._data.private_items[item] for item in range(self._num_items)]
        features = self._side.feature_matrix(items, device=self._ctx.device)     # row of private item i = the file of its public id
        replay = getattr(self._params, "sampler", "philox") == "replay"
        positives = self._data.i_train_dict if replay else self._data.sp_i_train
        self._sampler = custom_sampler.Sampler(positives, ctx=self._ctx, replay=replay)
        self._model = VBPRModel(self._factors, self._factors_d, self._learning_rate, self._l_w, self._l_b, self._l_e,
                                self._side.visual_features_shape, self._num_users, self._num_items, self._seed, ctx=self._ctx,
                                features=features, init_weights=kwargs.get("init_weights"))

    @property
    def name(self):
        return "VBPR" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"

    def _epoch_events(self):
        """An epoch's samples: transactions // batch_size FULL batches of the one stream (VBPR.py:115-127)."""
        return (self._data.transactions // self._batch_size) * self._batch_size
