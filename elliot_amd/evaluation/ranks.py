"""The rank metrics of the reference -- AUC, GAUC, LAUC (elliot/evaluation/metrics/accuracy/AUC/{auc,gauc,lauc}.py) -- from the
positions of the held-out items in each user's complete ranking, in NumPy: the host restatement of el_rank.hip for the tests
and for Evaluator.eval.

  list       top_k(where(mask, preds, -inf), k = num_items): (score desc, index asc), masked items a -inf tail
  neg_u      num_items - len(train_dict[u]) - len(rel_u) + 1                                       auc.py:78
  term       (neg_u - r_p + p) / neg_u for the p-th relevant item found, at 0-based position r_p   auc.py:79-80
  AUC        mean of all terms of all users                                                        auc.py:86-89
  GAUC       mean over users of sum / len(rel_u)                                                   gauc.py:83, 91-94
  LAUC@c     mean over users of the sum over positions < c, / min(c, len(rel_u))                   lauc.py:81-83
With m found items the per-user sum is (m neg - sum r + m (m - 1) / 2) / neg: an integer numerator and one division.
"""
import numpy as np

NAMES = ("AUC", "GAUC", "LAUC")
N_SUMS = 6       # sum S, sum m, sum S / |rel|, sum S^c / min(c, |rel|), users with a relevant item, users with neg <= 0


def positions(scores, admissible, targets):
    """scores [n, I] (float32 | float64), admissible bool [n, I] or None (every item), targets = (indptr, indices) with one row
    per row of scores (ids ascending, ids >= I allowed).  For each target entry: the number of admissible items ahead of it by
    (score desc, index asc) -- a stable sort of the negated scores, -0.0 taken as +0.0 -- or -1 for an id >= I or a masked
    target.  int32, in the order of the CSR's entries."""
    scores = np.asarray(scores)
    n, I = scores.shape
    indptr, indices = targets
    out = np.full(int(indptr[n] - indptr[0]), -1, dtype=np.int32)
    for r in range(n):
        s = scores[r] + scores.dtype.type(0)
        order = np.argsort(-s, kind="stable")
        if admissible is not None:
            order = order[np.asarray(admissible[r], dtype=bool)[order]]
        place = np.full(I, -1, dtype=np.int64)
        place[order] = np.arange(order.shape[0])
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            t = int(indices[e])
            if 0 <= t < I:
                out[e - int(indptr[0])] = place[t]
    return out


def user_rows(pos, indptr, ratings, threshold, train_len, n_items, cutoff):
    """The per-user rows el_rank_metrics sums, float64 [n, 6]: S_u, m_u, S_u / |rel_u|, S_u^c / min(c, |rel_u|), [|rel_u| > 0],
    [|rel_u| > 0 and neg_u <= 0] (such a user has zeros elsewhere).  pos: one entry per entry of the CSR rows (indptr[0] first)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.shape[0] - 1
    rows = np.zeros((n, N_SUMS), dtype=np.float64)
    base = int(indptr[0])
    for u in range(n):
        a, b = int(indptr[u]) - base, int(indptr[u + 1]) - base
        rel = np.ones(b - a, dtype=bool) if ratings is None else np.asarray(ratings[a + base:b + base], dtype=np.float64) >= threshold
        nrel = int(rel.sum())
        if nrel == 0:
            continue
        neg = int(n_items) - int(train_len[u]) - nrel + 1
        if neg <= 0:
            rows[u, 5] = 1.0
            continue
        p = np.asarray(pos[a:b], dtype=np.int64)[rel]
        found = p[p >= 0]
        head = found[found < cutoff]
        m, mc = int(found.shape[0]), int(head.shape[0])
        S = float(m * neg - int(found.sum()) + m * (m - 1) // 2) / float(neg)
        Sc = float(mc * neg - int(head.sum()) + mc * (mc - 1) // 2) / float(neg)
        rows[u] = (S, float(m), S / float(nrel), Sc / float(min(cutoff, nrel)), 1.0, 0.0)
    return rows


def means(sums):
    """{"AUC", "GAUC", "LAUC"} from the six sums; {} when no user has a relevant item.  Raises where the reference divides by
    zero (a user whose train and relevant items leave no negative)."""
    if sums[5] != 0:
        raise ZeroDivisionError(f"AUC / GAUC / LAUC: {int(sums[5])} user(s) have neg_num <= 0 (num_items - train - relevant + 1)")
    if sums[4] == 0:
        return {}
    return {"AUC": float(sums[0] / sums[1]) if sums[1] else float("nan"), "GAUC": float(sums[2] / sums[4]),
            "LAUC": float(sums[3] / sums[4])}


def finish(pos, indptr, ratings, threshold, train_len, n_items, cutoff):
    """(values, sums): the three metrics at `cutoff` and the float64[6] sums behind them, from host positions."""
    sums = user_rows(pos, indptr, ratings, threshold, train_len, n_items, cutoff).sum(axis=0)
    return means(sums), sums
