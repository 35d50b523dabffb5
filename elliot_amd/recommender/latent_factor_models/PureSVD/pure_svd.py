"""PureSVD plugin (YAML key `PureSVD` / `external.PureSVD`) -- Performance of Recommender Algorithms on Top-N Recommendation
Tasks (Cremonesi, Koren & Turrin 2010).

Contract of elliot/recommender/latent_factor_models/PureSVD/pure_svd.py: hyper-parameter `factors` (10) and the base class's
`seed`; train() factorises the binary train matrix once and evaluates.  Extra optional key: `gpu`.

The reference's train_step (pure_svd_model.py:36-43: sklearn's randomized_svd at its defaults) becomes
ops.PureSvdDeviceState.build: the Gaussian start matrix is drawn on the host exactly as sklearn draws it
(RandomState(seed).normal, rounded to float32), the power iterations run on the device in fp64 (el_spmm_csr_f64 and
el_psvd_orth), the (factors + 10)-order eigenproblem of Z^T Z is solved on the host (numpy.linalg.eigh), the tables are
projected and sign-flipped on the device (el_psvd_project, el_psvd_signs) and rounded once to float32.  Deviations, all documented:
  * the normaliser between the power iterations is Cholesky-QR run twice, not LU / QR, and the small SVD goes through the
    eigenvalues of Z^T Z: the same subspace in exact arithmetic; user_vec item_vec^T agrees with the reference run in float64
    more closely than the reference's own float32 run does (tests/test_oracle_puresvd.py), not bit for bit;
  * `factors` < 1, `factors` + 10 > 256 and `factors` + 10 > min(users, items) are refused (ValueError); the reference
    degrades to a thinner basis in the last case;
  * a train matrix whose numerical rank is below `factors` + 10 is refused (ValueError naming the column at which the
    orthonormalisation refused the pivot); the pivot test is relative, so iterates too ill-conditioned for Cholesky-QR are
    refused with it; the reference's LU / QR tolerate both;
  * masked items never fill a short list: it is padded with (-1, -inf) where the reference lists -inf items;
  * no dense score row is formed on the host: scores are formed and selected per block of users by el_score_topk;
  * the device memory the build needs is checked before anything is allocated; too little is refused with a ValueError
    stating the bytes.
save_weights / load_weights pickle {'user_vec', 'item_vec'} -- the reference's keys, so its checkpoints load.
"""
from .... import ops
from ...base_recommender_model import BaseRecommenderModel, init_charger
from ...recommender_utils_mixin import RecMixin
from .pure_svd_model import PureSVDModel


class PureSVD(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        # the reference's _params_list, verbatim (pure_svd.py:46-48): `name` and every output file name depend on it
        self._params_list = [
            ("_factors", "factors", "factors", 10, None, None)
        ]
        self.autoset_params()
        self._ratings = self._data.train_dict
        ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = PureSVDModel(self._factors, self._data, self._seed, ctx)

    @property
    def name(self):
        return f"PureSVD_{self.get_params_shortcut()}"

    def predict(self, u: int, i: int):
        """The score of the public (user, item) pair."""
        return self._model.predict(u, i)

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.train_step()                      # no epochs: one factorisation
        self.evaluate()
