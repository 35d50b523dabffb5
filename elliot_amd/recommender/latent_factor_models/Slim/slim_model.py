"""Model half of Slim (slim_model.py: train, prepare_predictions, get_user_recs).

What the reference computes -- one sklearn ElasticNet.fit per item in a Python loop, the cut of every column, the dense
R.dot(W), a masked top-k per user -- is done on the device without the dense score matrix: ops.slim_build (el_slim_order,
el_slim_fit over blocks of target columns, el_slim_w) and, from SparseWModel, ops.knn_score_topk per block of users (DESIGN.md
§3.17).
"""
from .... import ops
from ...sparse_w_model import SparseWModel


class SlimModel(SparseWModel):

    def __init__(self, data, l1_ratio, alpha, neighborhood, random_seed, exclusion, ctx):
        super().__init__(data, ctx)
        self._l1_ratio = float(l1_ratio)
        self._alpha = float(alpha)
        self._neighborhood = int(neighborhood)
        self._seed = int(random_seed)
        self._exclusion = str(exclusion)
        self.n_iter = None

    def initialize(self):
        self._upload_ratings()
        csc, csc_vals = ops.slim_csc(self.ctx, self._urm())
        self._W, self._W_vals, self.n_iter = ops.slim_build(self.ctx, csc, csc_vals, self._alpha, self._l1_ratio, self._neighborhood,
                                                            self._seed, self._exclusion)

    def hyper_state(self):
        return {"_l1_ratio": self._l1_ratio, "_alpha": self._alpha, "_neighborhood": self._neighborhood, "_seed": self._seed,
                "_exclusion": self._exclusion}

    def set_hyper_state(self, saving_dict):
        self._l1_ratio, self._alpha = float(saving_dict["_l1_ratio"]), float(saving_dict["_alpha"])
        self._neighborhood, self._seed = int(saving_dict["_neighborhood"]), int(saving_dict["_seed"])
        self._exclusion = str(saving_dict["_exclusion"])
