"""Model half shared by iALS and WRMF (iALS_model.py:17-125, wrmf_model.py:17-101): fp64 X, Y in HBM, ALS half-steps on the device.

The reference's per-row loops (np.linalg.inv / spsolve) become el_als_gram + el_als_solve (ops.AlsDeviceState).
Deviations, all documented: rows are solved by Cholesky (agreement to ~1e-12, not bit for bit); the dataset's train matrix is
never written (the reference stores the confidences into data.sp_i_train in place); the dense [U, I] pred_mat is not kept --
scores are formed and selected per block by el_score_topk_f64, and a checkpoint holds pred_mat only when U * I <= 2^28.
"""
import numpy as np
import scipy.sparse as sp

from ... import ops
from ..device_model import DeviceModel

PRED_MAT_MAX = 1 << 28


def ials_confidence(alpha, epsilon, scaling):
    """The float32 confidence of a train entry, computed as iALS_model.py:25-29 computes C.data from the binary float32 matrix."""
    one = np.ones(1, np.float32)
    if scaling == "linear":
        c = 1.0 + alpha * one
    elif scaling == "log":
        c = 1.0 + alpha * np.log(1.0 + one / epsilon)
    else:                                          # neither branch: C stays the binary matrix
        c = one
    return c.astype(np.float32)[0]


def ials_weights(alpha, epsilon=1.0, scaling="linear"):
    """(c, w_A, w_b): w_A = f64(Cu - 1) (float32 arithmetic, :57), w_b = f64(Cu) (:59).  Refuses what the kernels cannot solve."""
    if scaling == "log" and not float(epsilon) > 0.0:
        raise ValueError(f"iALS: epsilon={epsilon} with scaling 'log' gives no finite confidence (epsilon must be > 0)")
    if float(alpha) < 0.0:
        raise ValueError(f"iALS: alpha={alpha} < 0 gives negative weights (the normal equations lose definiteness)")
    c = ials_confidence(alpha, epsilon, scaling)
    w_A = float((np.full(1, c, np.float32) - 1)[0])
    if not (np.isfinite(c) and w_A >= 0.0):
        raise ValueError(f"iALS: alpha={alpha}, epsilon={epsilon} ({scaling}) give the weight {w_A}: it must be finite and >= 0")
    return c, w_A, float(c)


def wrmf_weights(alpha):
    """(c, w_A, w_b) of WRMF: C = alpha * sp_i_train keeps float32 (:26); A gets Y^T diag(C_u) Y, the rhs Y^T (C_u + I) P_u with
    P_u = 1 where C_u != 0 (:44-50)."""
    if float(alpha) < 0.0:
        raise ValueError(f"WRMF: alpha={alpha} < 0 gives negative weights (the normal equations lose definiteness)")
    c = (alpha * np.ones(1, np.float32)).astype(np.float32)[0]
    if not np.isfinite(c):
        raise ValueError(f"WRMF: alpha={alpha} is not finite in float32")
    return c, float(c), (float(c) + 1.0 if c != 0 else 0.0)


def check_factors(factors):
    if int(factors) > ops._lib.EL_ALS_MAX_F or int(factors) < 1:
        raise ValueError(f"factors={factors} unsupported: the ALS kernels solve 1..{ops._lib.EL_ALS_MAX_F} factors")


class AlsModel(DeviceModel):
    """X, Y drawn as the reference draws them (np.random seeded with `seed`: X first, then Y, normal(scale=0.01)), trained by
    ops.AlsDeviceState with the Gram timing of the model (gram="fresh": iALS, "stale": WRMF)."""
    gram = "fresh"
    sparse_tables = False          # WRMF keeps X, Y as scipy CSR in its checkpoint

    def __init__(self, factors, data, reg, seed, c, w_A, w_b, ctx=None):
        check_factors(factors)
        self.ctx = ctx or ops.get_context(0)
        self._data = data
        self.user_num, self.item_num = data.num_users, data.num_items
        self._c = np.float32(c)
        rs = np.random.RandomState(seed)
        X = rs.normal(scale=0.01, size=(self.user_num, int(factors)))
        Y = rs.normal(scale=0.01, size=(self.item_num, int(factors)))
        R = sp.csr_matrix(data.sp_i_train)
        self.state = ops.AlsDeviceState(self.ctx, X, Y, R.indptr, R.indices, w_A, w_b, reg, gram=self.gram)
        self._restored_pred_mat = None

    def train_step(self):
        self.state.step()
        self._restored_pred_mat = None

    def prepare_predictions(self):
        """The reference forms the dense X Y^T here (iALS_model.py:111-112); the device scores per block in recommend()."""

    def recommend(self, mask, k, start, stop):
        return self.state.recommend(mask, k, start, stop)

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by."""
        return self.state.rank(mask, targets, start, stop)

    def confidence_matrix(self):
        C = sp.csr_matrix(self._data.sp_i_train, dtype=np.float32, copy=True)
        C.data[:] = self._c
        return C

    def get_model_state(self):
        X, Y = self.state.X.cpu().numpy(), self.state.Y.cpu().numpy()
        pred = X.dot(Y.T) if X.shape[0] * Y.shape[0] <= PRED_MAT_MAX else None
        if self.sparse_tables:
            X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
        return {"pred_mat": pred, "X": X, "Y": Y, "C": self.confidence_matrix()}

    def set_model_state(self, saving_dict):
        """Accepts the reference's checkpoint too (dense X, Y for iALS, scipy CSR for WRMF); pred_mat is not read back."""
        for key, dst in (("X", self.state.X), ("Y", self.state.Y)):
            m = saving_dict[key]
            m = m.toarray() if sp.issparse(m) else np.asarray(m)
            if m.shape != tuple(dst.shape):
                raise ValueError(f"checkpoint {key} has shape {m.shape}, the model expects {tuple(dst.shape)}")
            dst.copy_(ops.torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)))


class IalsModel(AlsModel):
    gram = "fresh"


class WrmfModel(AlsModel):
    gram = "stale"
    sparse_tables = True
