"""NumPy restatement of iALS / WRMF training and scoring (iALS_model.py, wrmf_model.py) with Cholesky solves.

What it restates: the fp32 weight rules (w_A, w_b per model), the Gram timing (iALS: X^T X of the new X; WRMF: X^T X taken at
the top of the step from the old X), iALS's warm-item skip, the initial draw, and the masked top-k of X Y^T.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp


def init_tables(seed, U, I, F):
    rs = np.random.RandomState(seed)
    X = rs.normal(scale=0.01, size=(U, F))
    Y = rs.normal(scale=0.01, size=(I, F))
    return X, Y


def half(G, indptr, indices, Y, w_A, w_b, lam, X, skip_empty=False):
    """X[r] = (G + w_A sum y y^T + lam I)^-1 (w_b sum y) for every row r of the pattern; X is updated in place and returned."""
    F = G.shape[0]
    eye = np.eye(F)
    for r in range(len(indptr) - 1):
        idx = indices[indptr[r]:indptr[r + 1]]
        if skip_empty and idx.shape[0] == 0:
            continue
        P = Y[idx]
        A = G + w_A * P.T.dot(P) + lam * eye
        b = w_b * P.sum(axis=0)
        L = np.linalg.cholesky(A)
        z = sla.solve_triangular(L, b, lower=True)
        X[r] = sla.solve_triangular(L.T, z, lower=False)
    return X


def orientations(indptr, indices, U, I):
    R = sp.csr_matrix((np.ones(len(indices)), np.asarray(indices), np.asarray(indptr)), shape=(U, I))
    R.sort_indices()
    Rt = R.T.tocsr()
    Rt.sort_indices()
    return R, Rt


def ials_step(X, Y, R, Rt, w_A, w_b, lam):
    X = half(Y.T.dot(Y), R.indptr, R.indices, Y, w_A, w_b, lam, X)
    Y = half(X.T.dot(X), Rt.indptr, Rt.indices, X, w_A, w_b, lam, Y, skip_empty=True)
    return X, Y


def wrmf_step(X, Y, R, Rt, w_A, w_b, lam, fresh_gram=False):
    """fresh_gram=True is the WRONG reading (X^T X of the new X in the item half): kept to show the fixtures tell them apart."""
    yTy, xTx = Y.T.dot(Y), X.T.dot(X)
    X = half(yTy, R.indptr, R.indices, Y, w_A, w_b, lam, X)
    if fresh_gram:
        xTx = X.T.dot(X)
    Y = half(xTx, Rt.indptr, Rt.indices, X, w_A, w_b, lam, Y)
    return X, Y


def topk(X, Y, excl, k):
    """get_user_recs over every user with allunrated_mask: (idx int32 [U, k], val float64 [U, k]) by (score desc, index asc);
    padded with (-1, -inf); also the scores [U, I] (fp64)."""
    S = X.dot(Y.T)
    U, I = S.shape
    idx = np.full((U, k), -1, np.int32)
    val = np.full((U, k), -np.inf)
    for u in range(U):
        ok = np.ones(I, bool)
        ok[excl[1][excl[0][u]:excl[0][u + 1]]] = False
        items = np.nonzero(ok)[0]
        s = S[u, items]
        order = np.lexsort((items, -s))[:k]
        idx[u, :len(order)] = items[order]
        val[u, :len(order)] = s[order]
    return idx, val, S


def fragile_users(S, excl, k, rel=1e-9):
    """Users whose k-th and (k+1)-th candidate scores differ by at most rel * max|score|: their lists may legitimately differ."""
    U, I = S.shape
    tol = rel * np.abs(S).max()
    out = np.zeros(U, bool)
    for u in range(U):
        ok = np.ones(I, bool)
        ok[excl[1][excl[0][u]:excl[0][u + 1]]] = False
        s = np.sort(S[u, ok])[::-1]
        if s.shape[0] > k and s[k - 1] - s[k] <= tol:
            out[u] = True
        # ties inside the list reorder it as well
        if s.shape[0] > 1 and np.any(np.abs(np.diff(s[:min(k + 1, s.shape[0])])) <= tol):
            out[u] = True
    return out
