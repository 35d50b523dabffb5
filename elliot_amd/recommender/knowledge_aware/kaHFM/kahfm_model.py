"""KAHFMModel on the MI355X -- counterpart of elliot/recommender/knowledge_aware/kaHFM/kahfm_model.py.

The reference's model is its BPRMF MFModel with one factor per knowledge-graph feature and TF-IDF start tables instead of normal
draws: `update_factors` (:133-164) is MFModel.update_factors line for line, `prepare_predictions` (:166-167) is
global_bias(0) + item_bias + P Q^T, the checkpoint has the same four keys.  So this is MFModel (level-scheduled el_bprsgd_apply,
el_score_topk_f64) started from `init_weights`; rows of hundreds to thousands of factors take the wide-row kernel.
"""
from ...latent_factor_models.BPRMF.BPRMF_model import MFModel


class KAHFMModel(MFModel):
    def __init__(self, data, init_weights, lr, user_regularization, bias_regularization, positive_item_regularization,
                 negative_item_regularization, ctx=None, hogwild=False):
        """init_weights: (P0 [U, nF], Q0 [I, nF], b0 [I]) -- ops.kahfm_init and zeros (kahfm_model.py:47-72)."""
        super().__init__(int(init_weights[0].shape[1]), data, lr, user_regularization, bias_regularization,
                         positive_item_regularization, negative_item_regularization, 42, ctx=ctx, hogwild=hogwild,
                         init_weights=init_weights)

    @property
    def name(self):
        return "KGMF"

    def get_factors(self):
        return self._factors
