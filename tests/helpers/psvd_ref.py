"""NumPy fp64 restatement of PureSVD as the device computes it, pinned to tests/golden/puresvd_ref.npz.

  plan          R = factors + 10; n_iter = 7 if factors < 0.1 min(U, I) else 4; the method runs on A^T when U < I
  start_matrix  RandomState(seed).normal(size=(M.shape[1], R)) rounded to float32 (the reference's matrix is float32)
  restate       n_iter times Q <- orth(M Q), Q <- orth(M^T Q); Q <- orth(M Q); Z = M^T Q; eigh(Z^T Z) -> U^, s;
                tables and svd_flip as ops.PureSvdDeviceState.build, orth = Cholesky-QR run twice
  spmm_ordered  a CSR x dense product in el_spmm_csr_f64's documented order (stored order, pieces, slots in order)
  topk / fragile  masked top-k by (score desc, index asc) and the users whose list the reference's float32 rounding decides
"""
import numpy as np
import scipy.sparse as sp

OVERSAMPLES = 10


def plan(U, I, factors):
    R = int(factors) + OVERSAMPLES
    n_iter = 7 if factors < 0.1 * min(U, I) else 4
    return R, n_iter, U < I


def start_matrix(n, R, seed):
    return np.random.RandomState(seed).normal(size=(n, R)).astype(np.float32).astype(np.float64)


def csr_of(g, tag):
    """The binary float32 CSR of a golden case."""
    shape = tuple(int(x) for x in g[f"{tag}_shape"])
    indices = g[f"{tag}_indices"].astype(np.int32)
    return sp.csr_matrix((np.ones(indices.shape[0], np.float32), indices, g[f"{tag}_indptr"].astype(np.int64)), shape=shape)


def ref64_tables(g, tag, A):
    """(user_vec, item_vec * diag) of the reference's float64 run, rebuilt from the stored orthonormal table T = Q U^ over the rows
    of M and the identity diag(s) Vt = T^T M of the method: U >= I: user = T, item = A^T T; U < I: item = T s, user = A T / s.
    The error of the rebuilt P against the reference's own is recorded in the file (<tag>_rebuild_err)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    T = np.asarray(g[f"{tag}_t64"], np.float64)
    s = np.asarray(g[f"{tag}_sigma64"], np.float64)
    if A.shape[0] >= A.shape[1]:
        return T, np.asarray(A.T @ T)
    return np.asarray(A @ T) / s[None, :], T * s[None, :]


def ref32_lists(g, tag):
    """Every user's masked top-10 under the reference's float32 tables (stored as its differences from the float64 run's)."""
    top = g[f"{tag}_top64"].astype(np.int32).copy()
    top[g[f"{tag}_top32_rows"]] = g[f"{tag}_top32_lists"]
    return top


def cholqr(Y):
    G = Y.T @ Y
    L = np.linalg.cholesky(G)                              # raises LinAlgError on a non-positive pivot
    return np.linalg.solve(L, Y.T).T                       # Y L^-T


def orth(Y):
    return cholqr(cholqr(Y))


def flip_signs(T):
    """svd_flip: +1 / -1 per column from the entry of largest magnitude (numpy.argmax: the first one among equals)."""
    rows = np.argmax(np.abs(T), axis=0)
    return np.where(T[rows, np.arange(T.shape[1])] < 0, -1.0, 1.0)


def restate(A, factors, seed):
    """-> dict(user64, item64, user32, item32, sigma): the tables in fp64, rounded once to float32, and the singular values."""
    A = sp.csr_matrix(A, dtype=np.float64)
    U, I = A.shape
    R, n_iter, transposed = plan(U, I, factors)
    M = A.T.tocsr() if transposed else A
    Mt = M.T.tocsr()
    Q = start_matrix(M.shape[1], R, seed)
    for _ in range(n_iter):
        Q = orth(M @ Q)
        Q = orth(Mt @ Q)
    Q = orth(M @ Q)
    Z = Mt @ Q
    lam, vec = np.linalg.eigh(Z.T @ Z)
    order = np.argsort(lam)[::-1][:factors]
    s = np.sqrt(np.maximum(lam[order], 0.0))
    Uh = vec[:, order]
    if transposed:
        user, item = Z @ (Uh / s[None, :]), Q @ (Uh * s[None, :])
    else:
        user, item = Q @ Uh, Z @ Uh
    sg = flip_signs(user)                                  # the reference decides on U_M, or on the rows of Vt when transposed:
    user, item = user * sg[None, :], item * sg[None, :]    # the user-side table either way
    return dict(user64=user, item64=item, user32=user.astype(np.float32), item32=item.astype(np.float32), sigma=s)


def scores(user, item):
    return np.asarray(user, np.float64) @ np.asarray(item, np.float64).T


def spmm_ordered(indptr, indices, vals, X, piece_len):
    """Y = A X exactly as el_spmm_csr_f64 adds it: a row of at most piece_len entries from +0 in stored order; a longer row
    piece by piece, each piece from +0 in stored order, then the pieces from +0 in piece order."""
    n = indptr.shape[0] - 1
    X = np.asarray(X, np.float64)
    Y = np.zeros((n, X.shape[1]), np.float64)

    def run(a, b):
        acc = np.zeros(X.shape[1], np.float64)
        for e in range(a, b):
            v = np.float64(vals[e]) if vals is not None else np.float64(1.0)
            acc = acc + v * X[indices[e]]
        return acc

    for r in range(n):
        a, b = int(indptr[r]), int(indptr[r + 1])
        if b - a <= piece_len:
            Y[r] = run(a, b)
        else:
            acc = np.zeros(X.shape[1], np.float64)
            for p0 in range(a, b, piece_len):
                acc = acc + run(p0, min(p0 + piece_len, b))
            Y[r] = acc
    return Y


def topk(S, indptr, indices, k):
    """Masked top-k of every row of S by (score desc, index asc): (idx int32 [U, k], val float64 [U, k]), short rows padded with
    (-1, -inf); the items of CSR row u are masked."""
    U, I = S.shape
    idx = np.full((U, k), -1, np.int32)
    val = np.full((U, k), -np.inf, np.float64)
    for u in range(U):
        ok = np.ones(I, bool)
        ok[indices[indptr[u]:indptr[u + 1]]] = False
        items = np.flatnonzero(ok)
        s = S[u, items].astype(np.float64)
        order = np.lexsort((items, -s))[:k]
        idx[u, :len(order)] = items[order]
        val[u, :len(order)] = s[order]
    return idx, val


def fragile(S, row_err, indptr, indices, k):
    """Users whose top k + 1 masked scores under S hold a gap no larger than four times the row's largest |P_ref32 - P_ref64|
    (row_err) -- the rule of tests/test_gpu_ease_plugin.py: the gap between the k-th and the (k + 1)-th score decides who is
    in the list, the gaps above it decide the order inside it, and the lists are compared in order.  Their list is decided by
    the reference's float32 rounding."""
    out = np.zeros(S.shape[0], bool)
    for u in range(S.shape[0]):
        s = np.asarray(S[u], np.float64).copy()
        s[indices[indptr[u]:indptr[u + 1]]] = -np.inf
        top = np.sort(s[np.isfinite(s)])[::-1][:k + 1]
        out[u] = top.size > 1 and np.min(-np.diff(top)) <= 4.0 * row_err[u]
    return out
