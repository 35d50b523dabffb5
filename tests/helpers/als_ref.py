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


def backward_error(indptr, indices, Y, w_A, w_b, lam, X, rows=None):
    """Per row r (all rows, or those of `rows`, in that order): eta_r = |b_r - A_r x_r|_inf / (|A_r|_inf |x_r|_inf + |b_r|_inf) with
    A_r = Y^T Y + w_A sum y y^T + lam I and b_r = w_b sum y built from Y in np.longdouble -- the Gram too -- and x_r = X[r];
    0 where the denominator is 0.  The normwise backward error of x_r as a solution of the row's normal equations: it depends on
    the order of no sum and on no other solver.  A NaN in x_r gives NaN."""
    ld = np.longdouble
    Yl = np.asarray(Y, dtype=ld)
    F = Yl.shape[1]
    G = Yl.T.dot(Yl)
    lamI = ld(lam) * np.eye(F, dtype=ld)
    rows = range(len(indptr) - 1) if rows is None else rows
    eta = np.zeros(len(rows), dtype=np.float64)
    for n, r in enumerate(rows):
        P = Yl[indices[indptr[r]:indptr[r + 1]]]
        A = G + ld(w_A) * P.T.dot(P) + lamI
        b = ld(w_b) * P.sum(axis=0)
        x = np.asarray(X[r], dtype=ld)
        den = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
        if den != 0:                                      # (a NaN denominator is not 0: eta is NaN)
            eta[n] = float(np.abs(b - A.dot(x)).max() / den)
    return eta


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
