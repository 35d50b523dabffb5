"""NumPy / scipy restatement of the attribute kernels' contract (elliot_amd/csrc/el_attr.hip, el_knn.hip, include/elliot_hip.h).

  profile   one fp64 cell per (user, feature), the user's items in stored (train_dict) order:
            ADD   cell = cell + w from 0 per item that carries the feature, w = 1 / len (by_len) or 1
            LAST  cell = the weight in the last item that carries the feature, then cell / len (by_len)
            an entry per feature touched (zeros kept), columns ascending, float32(cell)
  dot[c,x]  = sum_t A[c,t] A[x,t] in fp64, added in row c's stored (ascending) order: scipy's own csr_matmat on the fp64 copy
  n_c       = sum_t A[c,t]^2, likewise
  dot       = float32(dot);  cosine = float32(dot / sqrt(n_c * n_x))
  top-N     = entries with dot != 0 and value != 0 by (value desc, index asc), self-similarity kept
  W         = csc(columns = targets).tocsr(), columns ascending
  VSM       = rows of both matrices divided by their fp64 norm, rounded once; scores = scipy's float32 csr_matmat
Scores and top-k of the attribute KNN models are knn_ref.scores / knn_ref.topk (scipy's float32 csr_matmat).
"""
import numpy as np
import scipy.sparse as sp


def profile_matrix(r_indptr, r_indices, F, weights, mode, by_len):
    """[U, nF] float32 CSR.  F: scipy CSR [I, nF] (features of every item, any order); weights: float64 per entry of F (LAST)."""
    U, nF = len(r_indptr) - 1, F.shape[1]
    indptr, cols, vals = [0], [], []
    for u in range(U):
        items = r_indices[r_indptr[u]:r_indptr[u + 1]]
        n = np.float64(len(items))
        w = np.float64(1.0) / n if by_len and len(items) else np.float64(1.0)
        cell = {}
        for i in items:
            for e in range(F.indptr[i], F.indptr[i + 1]):
                f = int(F.indices[e])
                if mode == "add":
                    cell[f] = cell.get(f, np.float64(0.0)) + w
                else:
                    cell[f] = np.float64(weights[e])
        for f in sorted(cell):
            cols.append(f)
            vals.append(cell[f] / n if (mode == "last" and by_len) else cell[f])
        indptr.append(len(cols))
    return sp.csr_matrix((np.asarray(vals, np.float64).astype(np.float32), np.asarray(cols, np.int32), np.asarray(indptr, np.int64)),
                         shape=(U, nF))


def rows64(A):
    A = sp.csr_matrix(A, dtype=np.float32).astype(np.float64)
    A.sort_indices()
    return A


def norms(A64):
    rows = np.repeat(np.arange(A64.shape[0]), np.diff(A64.indptr))
    return np.bincount(rows, weights=A64.data * A64.data, minlength=A64.shape[0])     # sequential adds in stored order


def column_lists(A, cols, n_neighbors, sim):
    """Top-N (x, value) of the given target columns: list of (int32 x in rank order, float32 values)."""
    A64 = rows64(A)
    nrm = norms(A64)
    dot = (A64[cols] @ A64.T.tocsr()).tocsr()           # row j = target cols[j]: sums in the stored order of its row of A
    out = []
    for j, c in enumerate(cols):
        lo, hi = dot.indptr[j], dot.indptr[j + 1]
        x, d = dot.indices[lo:hi].astype(np.int64), dot.data[lo:hi]
        keep = d != 0
        x, d = x[keep], d[keep]
        if sim == "dot":
            val = d.astype(np.float32)
        elif sim == "cosine":
            val = (d / np.sqrt(nrm[c] * nrm[x])).astype(np.float32)
        else:
            raise ValueError(sim)
        keep = val != 0
        x, val = x[keep], val[keep]
        order = np.lexsort((x, -val.astype(np.float64)))[:n_neighbors]
        out.append((x[order].astype(np.int32), val[order]))
    return out


def build_w(A, n_neighbors, sim):
    """W (n x n float32 CSR, columns ascending), W[x, c] = similarity of x in c's top-N."""
    n = A.shape[0]
    lists = column_lists(A, np.arange(n), n_neighbors, sim)
    indptr = np.concatenate([[0], np.cumsum([len(l[0]) for l in lists])]).astype(np.int64)
    rows = np.concatenate([l[0] for l in lists]) if n else np.zeros(0, np.int32)
    data = np.concatenate([l[1] for l in lists]) if n else np.zeros(0, np.float32)
    W = sp.csc_matrix((data, rows, indptr), shape=(n, n), dtype=np.float32).tocsr()
    W.sort_indices()
    return W


def normalize_rows(M):
    """Rows divided by their fp64 norm (sum of squares added in stored order), rounded once to float32; zero rows stay."""
    M = sp.csr_matrix(M, dtype=np.float32)
    d = M.data.astype(np.float64)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    norm = np.sqrt(np.bincount(rows, weights=d * d, minlength=M.shape[0]))
    norm[norm == 0] = 1.0
    out = sp.csr_matrix(((d / norm[rows]).astype(np.float32), M.indices, M.indptr), shape=M.shape)
    out.sort_indices()
    return out


def vsm_scores(user_profiles, item_profiles):
    """VSM's dense float32 scores: both matrices row-normalised once, then scipy's own float32 csr_matmat."""
    B = normalize_rows(item_profiles).T.tocsr()
    B.sort_indices()
    return np.asarray(normalize_rows(user_profiles).dot(B).toarray(), dtype=np.float32)


def bound(L):
    """Relative distance allowed between the reference's float32 similarity and the fp64 one rounded once: the reference normalises
    two rows of at most L float32 terms and adds an L-term float32 dot product ((2 L + 8) roundings of 2^-24 cover the sums, the two
    square roots, the divisions and our own final rounding)."""
    return (2 * L + 8) * 2.0 ** -24


def compare_columns(ref_lists, our_lists, rtol, n_neighbors):
    """The checks of one W against the reference's, column by column: equal lengths; ALL values, sorted descending, agree entry
    by entry within rtol; the index sets agree on the entries whose value exceeds the column's cut value by more than 2 rtol
    (a column shorter than n_neighbors is not cut: its index sets are equal).
    Returns (entries compared by index, entries in all)."""
    strict = total = 0
    for c, ((rx, rv), (ox, ov)) in enumerate(zip(ref_lists, our_lists)):
        assert len(rx) == len(ox), (c, len(rx), len(ox))
        if not len(rx):
            continue
        r_order = np.lexsort((rx, -rv.astype(np.float64)))
        rx, rv = rx[r_order], rv[r_order].astype(np.float64)
        ov64 = ov.astype(np.float64)
        assert np.all(np.abs(ov64 - rv) <= rtol * np.abs(rv)), (c, float(np.max(np.abs(ov64 - rv) / np.abs(rv))))
        if len(rx) < n_neighbors:
            assert set(rx.tolist()) == set(ox.tolist()), c
            strict, total = strict + len(rx), total + len(rx)
            continue
        cut = min(rv.min(), ov64.min())
        far_r = rv > cut * (1 + 2 * rtol) if cut > 0 else rv > cut
        far_o = ov64 > cut * (1 + 2 * rtol) if cut > 0 else ov64 > cut
        assert set(rx[far_r].tolist()) <= set(ox.tolist()) and set(ox[far_o].tolist()) <= set(rx.tolist()), c
        strict += int(min(far_r.sum(), far_o.sum()))
        total += len(rx)
    return strict, total
