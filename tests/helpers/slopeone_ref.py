"""SlopeOne restated in vectorised NumPy / SciPy: what scripts/gen_golden_slopeone.py proves equal, bit for bit, to the reference's
SlopeOneModel (initialize, predict, get_user_recs) before it writes tests/golden/slopeone_ref.npz.  TEST INFRASTRUCTURE: the
tests compare the kernels with this; it reads arrays (the golden file's or a test's own), never the reference checkout.

Ratings are integers or half steps, so every sum below is an exact integer (ratings times 2) and no order matters until the
prediction's chain, which is taken left to right in the stored (dict) order of the user's row."""
import numpy as np
import scipy.sparse as sp


def case(g, tag):
    """(indptr, indices, ratings, U, I) of one case of the golden file: rows in the reference's dict order."""
    U, I = (int(x) for x in g[f"{tag}_shape"])
    return g[f"{tag}_indptr"], g[f"{tag}_indices"], g[f"{tag}_ratings"], U, I


def _matrices(indptr, indices, ratings, U, I):
    r2 = np.asarray(ratings, dtype=np.float64) * 2.0
    assert np.array_equal(r2, np.round(r2)), "integer or half-step ratings only"
    M = sp.csr_matrix((r2.astype(np.int64), np.asarray(indices, dtype=np.int64), np.asarray(indptr, dtype=np.int64)), shape=(U, I))
    B = sp.csr_matrix((np.ones(M.nnz, np.int64), M.indices, M.indptr), shape=(U, I))
    return M.tocsc(), B.tocsc()


def build_rows(indptr, indices, ratings, U, I, rows):
    """(freq[rows, :], dev[rows, :]) as float64: slope_one_model.py:19-34 with freq and dev started from zero."""
    M, B = _matrices(indptr, indices, ratings, U, I)
    rows = np.asarray(rows, dtype=np.int64)
    freq = np.asarray((B[:, rows].T @ B).todense(), dtype=np.int64)                          # [n, I]
    S2 = np.asarray((M[:, rows].T @ B - B[:, rows].T @ M).todense(), dtype=np.int64)        # 2 * sum (r_uc - r_ux)
    f = freq.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        up_cx = np.where(freq != 0, (S2 * 0.5) / f, 0.0)          # dev[c, x] where c < x
        up_xc = np.where(freq != 0, (-S2 * 0.5) / f, 0.0)         # dev[x, c] where x < c; dev[c, x] is its negation
    x = np.arange(I)[None, :]
    c = rows[:, None]
    dev = np.where(x > c, up_cx, -up_xc)
    dev[x == c] = 0.0
    return f, dev


def build(indptr, indices, ratings, U, I):
    """(freq, dev, user_mean): float64 [I, I] twice and float64 [U] (nan for a user without ratings, as np.mean of nothing)."""
    freq, dev = build_rows(indptr, indices, ratings, U, I, np.arange(I))
    return freq, dev, user_mean(indptr, ratings)


def user_mean(indptr, ratings):
    """np.mean of every row: the sums are exact, so any order of addition gives np.mean's result."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = np.diff(indptr)
    s = np.add.reduceat(np.concatenate([np.asarray(ratings, dtype=np.float64), [0.0]]), np.minimum(indptr[:-1], len(ratings)))
    s[n == 0] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / n


def table(freq, dev):
    """T[j, i] = dev[i, j] where freq[i, j] > 0, NaN elsewhere."""
    return np.where(freq > 0, dev, np.nan).T.copy()


def predictions(indptr, indices, freq, dev, mean, users=None):
    """predict(u, i) for the given users (default: all) and every item: float64 [n, I].  s starts from +0 and takes dev[i, j]
    for the j of the row in stored order with freq[i, j] > 0, one addition each; mean + s / count, or mean when count == 0."""
    I = freq.shape[0]
    users = np.arange(len(indptr) - 1) if users is None else np.asarray(users)
    ok = freq > 0
    out = np.empty((len(users), I), dtype=np.float64)
    for r, u in enumerate(users):
        s = np.zeros(I, dtype=np.float64)
        cnt = np.zeros(I, dtype=np.int64)
        for j in indices[indptr[u]:indptr[u + 1]]:
            m = ok[:, j]
            s[m] = s[m] + dev[m, j]
            cnt += m
        with np.errstate(divide="ignore", invalid="ignore"):
            out[r] = np.where(cnt > 0, mean[u] + s / cnt, mean[u])
    return out


def topk(values, allowed, k):
    """(idx int32 [k], val float64 [k]) of one row: the allowed items by (value desc, index asc), padded with (-1, -inf);
    NaN values are never selected."""
    cand = np.flatnonzero(np.asarray(allowed) & ~np.isnan(values))
    order = cand[np.lexsort((cand, -values[cand]))][:k]
    idx = np.full(k, -1, np.int32)
    val = np.full(k, -np.inf, np.float64)
    idx[:len(order)] = order
    val[:len(order)] = values[order]
    return idx, val


def has_tie(values, allowed, k):
    """True when two equal values stand inside the top k or at its edge (positions k - 1 and k): the order the reference's
    argpartition leaves there is arbitrary."""
    v = np.sort(values[np.asarray(allowed)])[::-1][:k + 1]
    return bool(np.any(v[1:] == v[:-1]))
