"""VSM model (vector_space_model_similarity.py: Similarity): score[u, i] = cosine of user u's profile and item i's attribute row.

sklearn's cosine_similarity(user_profiles, item_profiles) normalises the rows of both matrices and multiplies them
(safe_sparse_dot: scipy's csr_matmat in float32).  Here the rows are normalised once on the host and the product is
el_knn_score_topk with A = the user profiles and B = the transposed item profiles (columns ascending): the same sums in the same
order, masked and cut to the top-k per user, without the [U, I] block.
"""
import numpy as np

from .... import ops
from ...device_model import DeviceModel
from ... import attribute_profiles as ap

SIMILARITIES = ("cosine",)


class Similarity(DeviceModel):

    def __init__(self, data, user_profile_matrix, item_attribute_matrix, similarity, ctx):
        """The two matrices are functions without arguments, called by initialize() only."""
        if similarity == "dot":
            raise ValueError("VSM: similarity 'dot' is not usable -- the reference's branch multiplies the rating matrix with "
                             f"itself and ignores both profiles.  Supported: {list(SIMILARITIES)}")
        if similarity not in SIMILARITIES:
            raise ValueError(f"VSM: value for parameter 'similarity' not recognized ({similarity!r}).  "
                             f"Supported: {list(SIMILARITIES)}")
        self._data, self.ctx = data, ctx
        self._user_profile_matrix, self._item_attribute_matrix = user_profile_matrix, item_attribute_matrix
        self._similarity = similarity
        self._A = self._B = None                          # host CSRs: normalised user profiles, transposed item profiles

    def _upload(self):
        dev = self.ctx.device
        self._Ad, self._Ad_vals = ops.DeviceCSR(self._A.indptr, self._A.indices, self._A.shape[1], dev), ops.device_values(self._A.data, dev)
        self._Bd, self._Bd_vals = ops.DeviceCSR(self._B.indptr, self._B.indices, self._B.shape[1], dev), ops.device_values(self._B.data, dev)

    def initialize(self):
        self._A = ap.sorted_csr(ap.l2_normalize_rows(self._user_profile_matrix()))
        self._B = ap.sorted_csr(ap.l2_normalize_rows(self._item_attribute_matrix()).T.tocsr())
        self._upload()

    def recommend(self, mask, k, start, stop):
        return ops.knn_score_topk(self.ctx, self._Ad, self._Ad_vals, self._Bd, self._Bd_vals, start, stop, k, **ops.mask_kwargs(mask))

    def get_model_state(self):
        out = {"_similarity": self._similarity}
        for tag, M in (("_A", self._A), ("_B", self._B)):
            out.update({f"{tag}_data": M.data, f"{tag}_indices": M.indices, f"{tag}_indptr": M.indptr,
                        f"{tag}_shape": np.asarray(M.shape, np.int64)})
        return out

    def set_model_state(self, saving_dict):
        import scipy.sparse as sp
        self._similarity = saving_dict["_similarity"]
        if "_A_indptr" not in saving_dict:                # the reference's checkpoint holds the similarity's name only
            return self.initialize()
        self._A, self._B = (sp.csr_matrix((saving_dict[f"{t}_data"], saving_dict[f"{t}_indices"], saving_dict[f"{t}_indptr"]),
                                          shape=tuple(saving_dict[f"{t}_shape"])) for t in ("_A", "_B"))
        self._upload()
