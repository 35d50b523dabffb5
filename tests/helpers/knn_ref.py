"""NumPy / scipy restatement of the ItemKNN / UserKNN contract (elliot_amd/csrc/el_knn.hip, include/elliot_hip.h).

  cnt[c, x] = sum_t r_tc r_tx, n_c = sum_t r_tc^2     exact in fp64 (integer or half-step ratings)
  dot       = float32(cnt)
  cosine    = float32(cnt / sqrt(n_c * n_x))           fp64, rounded once
  top-N     = non-zero values of column c by (value desc, index asc)
  W         = csc(columns = targets).tocsr(), columns ascending
  scores    = scipy's own R.dot(W) (ItemKNN) / W.dot(R) (UserKNN)
  top-k     = (score desc, index asc) over unmasked items, zero scores included, (-1, -inf) padding

Every function that a large-shape test needs works on a subset of columns or users, so the CPU side stays cheap.
"""
import numpy as np
import scipy.sparse as sp


def targets_matrix(R, side):
    """Rows = the targets of the similarity (items for ItemKNN, users for UserKNN), fp64."""
    R = sp.csr_matrix(R)
    M = R.T.tocsr() if side == "item" else R.copy()
    M = M.astype(np.float64)
    M.sort_indices()
    return M


def column_lists(M, cols, n_neighbors, sim):
    """Top-N (x, value) of the given target columns: list of (int32 x ascending-by-rank, float32 values)."""
    nrm = np.asarray(M.multiply(M).sum(axis=1)).ravel()
    cnt = (M @ M[cols].T).tocsc()                       # [n, len(cols)], exact integer-valued sums
    out = []
    for j, c in enumerate(cols):
        lo, hi = cnt.indptr[j], cnt.indptr[j + 1]
        x = cnt.indices[lo:hi].astype(np.int64)
        v = cnt.data[lo:hi]
        keep = v != 0
        x, v = x[keep], v[keep]
        if sim == "dot":
            val = v.astype(np.float32)
        elif sim == "cosine":
            val = (v / np.sqrt(nrm[c] * nrm[x])).astype(np.float32)
        else:
            raise ValueError(sim)
        order = np.lexsort((x, -val.astype(np.float64)))[:n_neighbors]
        out.append((x[order].astype(np.int32), val[order]))
    return out


def build_w(R, side, n_neighbors, sim):
    """W (n x n float32 CSR, columns ascending), W[x, c] = similarity of x in c's top-N."""
    M = targets_matrix(R, side)
    n = M.shape[0]
    lists = column_lists(M, np.arange(n), n_neighbors, sim)
    indptr = np.concatenate([[0], np.cumsum([len(l[0]) for l in lists])]).astype(np.int64)
    rows = np.concatenate([l[0] for l in lists]) if n else np.zeros(0, np.int32)
    data = np.concatenate([l[1] for l in lists]) if n else np.zeros(0, np.float32)
    W = sp.csc_matrix((data, rows, indptr), shape=(n, n), dtype=np.float32).tocsr()
    W.sort_indices()
    return W


def scores(R, W, side, users=None):
    """Dense fp32 score rows (scipy's csr_matmat, exactly what the reference computes) for `users` (all by default)."""
    R = sp.csr_matrix(R, dtype=np.float32)
    if users is None:
        users = np.arange(R.shape[0])
    if side == "item":
        P = R[users].dot(W)
    else:
        P = W[users].dot(R)
    return np.asarray(P.toarray(), dtype=np.float32)


def topk(preds, users, k, excl=None, cand=None):
    """preds [len(users), I]; excl / cand = (indptr, indices) over ALL users.  Returns idx int32 [n, k], val float32 [n, k]."""
    n, I = preds.shape
    idx = np.full((n, k), -1, np.int32)
    val = np.full((n, k), -np.inf, np.float32)
    for r, u in enumerate(users):
        if cand is not None:
            items = np.asarray(cand[1][cand[0][u]:cand[0][u + 1]], np.int64)
        else:
            ok = np.ones(I, bool)
            if excl is not None:
                ok[excl[1][excl[0][u]:excl[0][u + 1]]] = False
            items = np.nonzero(ok)[0]
        s = preds[r, items] + np.float32(0.0)
        order = np.lexsort((items, -s.astype(np.float64)))[:k]
        idx[r, :len(order)] = items[order]
        val[r, :len(order)] = s[order]
    return idx, val


def cut_ties_equal(idx_a, val_a, idx_b, val_b):
    """Index lists equal except where the value is tied (the reference's unstable argsort / argpartition)."""
    if not np.array_equal(val_a, val_b):
        return False
    for ra, rb, va in zip(idx_a, idx_b, val_a):
        for v in np.unique(va):
            if set(ra[va == v].tolist()) != set(rb[va == v].tolist()):
                # the last tied group may be cut differently: allowed only for the lowest value in the row
                if v != va.min():
                    return False
    return True
