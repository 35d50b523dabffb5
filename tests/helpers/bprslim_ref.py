"""BPRSlim restated in NumPy: what scripts/gen_golden_bprslim.py proves equal, bit for bit, to the reference's BPRSlimModel
(train_step, predict, get_user_recs) before it writes tests/golden/bprslim_ref.npz.  TEST INFRASTRUCTURE: the tests compare the
kernels with this; it reads arrays (the golden file's or a test's own), never the reference checkout.

The rows a step and a prediction walk are those of the reference's scipy train matrix: every row in ascending item id
(`sorted_rows`).  The golden file stores the rows in the order of the train dict, which is what the replayed sampler needs."""
import math

import numpy as np

CASES = ("plain", "short_rows", "defaults")


def case(g, tag):
    """(indptr, indices, U, I) of one case of the golden file: rows in the reference's dict order."""
    U, I = (int(x) for x in g[f"{tag}_shape"])
    return g[f"{tag}_indptr"], g[f"{tag}_indices"], U, I


def hyper(g, tag):
    lr, lj_reg, li_reg = (float(x) for x in g[f"{tag}_hyper"])
    return {"lr": lr, "lj_reg": lj_reg, "li_reg": li_reg}


def sorted_rows(indptr, indices):
    """The same rows, each in ascending item id: the order scipy's CSR holds them in."""
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.asarray(indices, dtype=np.int32).copy()
    for a, b in zip(indptr[:-1], indptr[1:]):
        out[a:b] = np.sort(out[a:b])
    return indptr, out


def step(S, row, i, j, lr, li_reg, lj_reg, chain="left"):
    """train_step (bprslim_model.py:36-67) of one triplet on S in place; returns x_uij.  chain: "left" is the reference's
    left-to-right fp64 chain of rounded differences, "fsum" the correctly rounded sum of the same rounded differences."""
    d = S[i, row] - S[j, row]
    if chain == "fsum":
        x = math.fsum(d.tolist())
    else:
        x = 0.0
        for v in d.tolist():
            x += v
    g = 1 / (1 + np.exp(x))
    for s in row.tolist():
        if s != i:
            S[i, s] += lr * (g - li_reg * S[i, s])
        if s != j:
            S[j, s] -= lr * (g - lj_reg * S[j, s])
    return x


def train(S, indptr, indices, trip, lr, li_reg, lj_reg, chain="left"):
    """Every triplet of trip (int [3, n]: u, i, j) in order on S in place (rows ascending); returns x float64 [n]."""
    x = np.empty(trip.shape[1], dtype=np.float64)
    for t, (u, i, j) in enumerate(trip.T.tolist()):
        x[t] = step(S, indices[indptr[u]:indptr[u + 1]], i, j, lr, li_reg, lj_reg, chain)
    return x


def predictions(indptr, indices, S, users=None):
    """predict(u, i) (bprslim_model.py:69-84) for the given users (default: all) and every item: float64 [n, I], one addition
    per seen item from +0, in stored order."""
    I = S.shape[0]
    users = np.arange(len(indptr) - 1) if users is None else np.asarray(users)
    out = np.zeros((len(users), I), dtype=np.float64)
    for r, u in enumerate(users):
        for s in indices[indptr[u]:indptr[u + 1]]:
            out[r] = out[r] + S[:, s]
    return out


def levels(i, j, I):
    """(level int [n] from 1, order, level_start) of a triplet sequence: a triplet follows the last earlier one that shares row
    i or row j of S; the order within a level is the sequence's."""
    last = np.zeros(I, dtype=np.int64)
    lev = np.empty(len(i), dtype=np.int64)
    for t, (a, b) in enumerate(zip(np.asarray(i).tolist(), np.asarray(j).tolist())):
        lev[t] = max(last[a], last[b]) + 1
        last[a] = last[b] = lev[t]
    order = np.argsort(lev, kind="stable").astype(np.int32)
    n_levels = int(lev.max()) if len(lev) else 0
    start = np.concatenate([[0], np.cumsum(np.bincount(lev, minlength=n_levels + 1)[1:])]).astype(np.int64)
    return lev, order, start


def topk(values, allowed, k):
    """(idx int32 [k], val float64 [k]) of one row: the allowed items by (value desc, index asc), padded with (-1, -inf)."""
    cand = np.flatnonzero(np.asarray(allowed))
    order = cand[np.lexsort((cand, -values[cand]))][:k]
    idx = np.full(k, -1, np.int32)
    val = np.full(k, -np.inf, np.float64)
    idx[:len(order)] = order
    val[:len(order)] = values[order]
    return idx, val


def min_gap(values, allowed, k):
    """The smallest difference between neighbours among the k + 1 largest allowed values (inf with fewer than two): 0 is a tie
    inside or at the edge of the top k."""
    v = np.sort(values[np.asarray(allowed)])[::-1][:k + 1]
    return float(np.min(v[:-1] - v[1:])) if len(v) > 1 else float("inf")
