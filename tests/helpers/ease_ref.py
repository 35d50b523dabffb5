"""NumPy restatement of EASE^R (ease_r.py:70-93) as the device computes it, pinned to tests/golden/ease_ref.npz.

  gram     G = R^T R, exact integer sums in float64, diagonal (float)(n_i + l2_norm) with n_i = stored entries of column i
  weights  P = G^-1 in float64, B[j, i] = (float)(-P[j, i] / P[i, i]), B[i, i] = 0
  scores   R.dot(B) with scipy (float32 CSR x float32 dense: the reference's own product)
  topk     masked top-k by (score desc, index asc), rows short of k padded with (-1, -inf)
"""
import numpy as np
import scipy.sparse as sp


def gram(R, l2_norm):
    R = sp.csr_matrix(R, dtype=np.float64)
    G = (R.T @ R).toarray()
    n = np.diff(sp.csc_matrix(R).indptr)
    G[np.diag_indices(G.shape[0])] = (n + float(l2_norm)).astype(np.float32).astype(np.float64)
    return G


def weights(P):
    """B from an fp64 inverse P: one correctly rounded division, one rounding to float32."""
    B = (-P / np.diag(P)[None, :]).astype(np.float32)
    B[np.diag_indices(B.shape[0])] = 0.0
    return B


def weights_f64(R, l2_norm):
    return weights(np.linalg.inv(gram(R, l2_norm)))


def scores(R, B):
    return sp.csr_matrix(R, dtype=np.float32).dot(np.asarray(B, dtype=np.float32))


def topk(S, excl, k, cand=None):
    """excl: (indptr, indices) of the items to leave out of every row; cand: the same, of the only items allowed."""
    U, I = S.shape
    idx = np.full((U, k), -1, np.int32)
    val = np.full((U, k), -np.inf, np.float32)
    for u in range(U):
        ok = np.ones(I, bool)
        if excl is not None:
            ok[excl[1][excl[0][u]:excl[0][u + 1]]] = False
        if cand is not None:
            c = np.zeros(I, bool)
            c[cand[1][cand[0][u]:cand[0][u + 1]]] = True
            ok &= c
        items = np.flatnonzero(ok)
        s = S[u, items] + np.float32(0.0)
        order = np.lexsort((items, -s.astype(np.float64)))[:k]
        idx[u, :len(order)] = items[order]
        val[u, :len(order)] = s[order]
    return idx, val


def same_lists(ref_idx, idx, S):
    """Per row: does (idx) agree with the reference's list?  Every rank must name an item with the score of the reference's item
    at that rank under S, and the same item wherever that score is not tied in the row (the reference's argpartition orders
    ties arbitrarily)."""
    ok = np.ones(ref_idx.shape[0], bool)
    for u in range(ref_idx.shape[0]):
        keep = ref_idx[u] >= 0
        if not np.array_equal(keep, idx[u] >= 0):
            ok[u] = False
            continue
        for r in np.flatnonzero(keep):
            s = S[u, ref_idx[u, r]]
            tied = np.count_nonzero(S[u] == s) > 1
            if idx[u, r] != ref_idx[u, r] and (not tied or S[u, idx[u, r]] != s):
                ok[u] = False
                break
    return ok
