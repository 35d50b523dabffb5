"""Model half of RP3beta (rp3beta.py: train, get_user_predictions).

What the reference computes -- two normalised operands, the dense item-item product in blocks of 200 rows, a cut of every row
and of every column, the block R.dot(W), a masked top-k per user -- is done on the device without the dense product and without
the [U, I] score block: ops.rp3_operands (el_csr_row_l1; the two powers stay NumPy's, on the host), ops.rp3_build (el_rp3_rows,
el_rp3_cut) and, from SparseWModel, ops.knn_score_topk per block of users.
"""
from .... import ops
from ...sparse_w_model import SparseWModel


class RP3betaModel(SparseWModel):

    def __init__(self, data, neighborhood, alpha, beta, normalize_similarity, ctx):
        super().__init__(data, ctx)
        self._neighborhood = int(neighborhood)
        self._alpha = float(alpha)
        self._beta = float(beta)
        self._normalize_similarity = bool(normalize_similarity)

    def initialize(self):
        self._upload_ratings()
        operands = ops.rp3_operands(self.ctx, self._urm(), self._alpha, self._beta)
        self._W, self._W_vals = ops.rp3_build(self.ctx, *operands, self._neighborhood, self._normalize_similarity)

    def hyper_state(self):
        return {"_neighborhood": self._neighborhood, "_alpha": self._alpha, "_beta": self._beta,
                "_normalize_similarity": self._normalize_similarity}

    def set_hyper_state(self, saving_dict):
        self._neighborhood = int(saving_dict["_neighborhood"])
        self._alpha, self._beta = float(saving_dict["_alpha"]), float(saving_dict["_beta"])
        self._normalize_similarity = bool(saving_dict["_normalize_similarity"])
