"""Per-user reference of the accuracy metrics (el_rec_metrics) and of the fragile-user bound (el_topk_fragile), in plain Python:
no device code and nothing taken from Evaluator._eval_accuracy.  The definitions are those of the header comment of
csrc/el_metrics.hip, one user at a time, with correctly rounded sums (math.fsum):

  relevant   the user's test items with rating >= thr (rating 1.0 for every item when there are no ratings); items the model's
             catalogue does not hold still count
  gain       2.0 ** (rating - thr + 1) - 1 on the float32 rating widened to a Python float
  discount   math.log(2) / math.log(rank + 2), rank 0-based
  nDCG       DCG / IDCG: DCG = sum of gain x discount over the hits of the first `cutoff` slots, IDCG = the same sum over the
             min(cutoff, #relevant) largest gains in descending order; 0 when either is 0
  Precision  hits / cutoff        Recall  hits / #relevant        HR  1 when there is a hit
  MAP        (sum over ranks r = 1..cutoff of (hits within the first r slots) / r) / cutoff
  MRR        1 / (1-based rank of the first hit)
  F1         2 * Precision * Recall / (Precision + Recall), 0 when both are 0
  valid      1 when the user has a relevant item; every other column of a user without one is 0

A -1 slot keeps its rank and never hits; a recommended item that appears twice hits twice.  Columns: METRIC_NAMES + valid."""
import math
from types import SimpleNamespace

import numpy as np

NAMES = ("nDCG", "Precision", "Recall", "HR", "MAP", "MRR", "F1")


def rows(recs, indptr, items, ratings, thr, cutoff, u_start=0):
    """float64[n, 8] for the users u_start .. u_start + n of the test CSR, n = len(recs)."""
    recs = np.asarray(recs)
    n = recs.shape[0]
    out = np.zeros((n, 8), np.float64)
    disc = [math.log(2) / math.log(r + 2) for r in range(cutoff)]
    thr = float(thr)
    for q in range(n):
        a, b = int(indptr[u_start + q]), int(indptr[u_start + q + 1])
        rel = {}
        for e in range(a, b):
            r = float(np.float32(ratings[e])) if ratings is not None else 1.0
            if r >= thr:
                rel[int(items[e])] = 2.0 ** (r - thr + 1) - 1
        if not rel:
            continue
        best = sorted(rel.values(), reverse=True)[:cutoff]
        idcg = math.fsum(g * disc[t] for t, g in enumerate(best))
        hits = [int(it) >= 0 and int(it) in rel for it in recs[q, :cutoff]]
        dcg = math.fsum(rel[int(it)] * disc[c] for c, it in enumerate(recs[q, :cutoff]) if hits[c])
        nh, terms = 0, []
        for c, h in enumerate(hits):
            nh += h
            terms.append(nh / (c + 1))
        prec, rcl = nh / cutoff, nh / len(rel)
        out[q, 0] = dcg / idcg if dcg > 0 and idcg > 0 else 0.0
        out[q, 1] = prec
        out[q, 2] = rcl
        out[q, 3] = 1.0 if nh else 0.0
        out[q, 4] = math.fsum(terms) / cutoff
        out[q, 5] = 1.0 / (hits.index(True) + 1) if nh else 0.0
        out[q, 6] = 2.0 * prec * rcl / (prec + rcl) if prec + rcl > 0 else 0.0
        out[q, 7] = 1.0
    return out


def sums(rws):
    """float64[8]: the correctly rounded column sums over the rows with column 7 non-zero."""
    v = rws[rws[:, 7] != 0]
    return np.array([math.fsum(v[:, m].tolist()) for m in range(8)], np.float64)


def means(rws):
    s = sums(rws)
    return {n: s[m] / s[7] for m, n in enumerate(NAMES)} if s[7] else {}


# ---- shared cases ------------------------------------------------------------------------------------------------------
RANDOM_CASES = [(10, 0.0, False), (50, 3.0, False), (100, 2.5, True), (7, 1.0, True)]      # cutoff, thr, fractional ratings


def random_case(cutoff, frac_ratings):
    """700 users, 4000 items, degrees 0..29 with one 1500-item row and one empty row, planted hits and some -1 slots:
    (recs int32[U, k], indptr, items, ratings float32)."""
    rs = np.random.RandomState(cutoff)
    U, I, k = 700, 4000, max(cutoff, 20)
    deg = rs.randint(0, 30, size=U)
    deg[5] = 1500                                   # > LDS gain buffer: chunked selection of the IDCG gains
    deg[6] = 0
    ip = np.zeros(U + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    items = np.concatenate([np.sort(rs.choice(I, size=d, replace=False)) for d in deg]).astype(np.int32)
    ratings = (rs.uniform(0.5, 5.0, size=ip[-1]) if frac_ratings else rs.randint(1, 6, size=ip[-1])).astype(np.float32)
    recs = np.stack([rs.choice(I, size=k, replace=False) for _ in range(U)]).astype(np.int32)
    for u in range(0, U, 3):                        # plant hits
        if deg[u]:
            row = items[ip[u]:ip[u + 1]]
            pos = rs.choice(k, size=min(3, len(row), k), replace=False)
            pick = rs.choice(row, size=len(pos), replace=False)
            keep = ~np.isin(recs[u], pick)
            recs[u] = np.where(keep, recs[u], (recs[u] + I) % (2 * I) + I)   # drop accidental duplicates of the planted ids
            recs[u][pos] = pick
    recs[recs >= I] = -1                            # some empty slots too
    return recs, ip, items, ratings


def evaluator_means(recs_idx, ip, items, ratings, thr, cutoff):
    """The means of the host Evaluator (elliot_amd.evaluation.evaluator) for the same case, by metric name."""
    from elliot_amd.dataset.dataset import default_config
    from elliot_amd.evaluation.evaluator import Evaluator
    U, k = recs_idx.shape
    test = {u: {int(i): float(r) for i, r in zip(items[ip[u]:ip[u + 1]], ratings[ip[u]:ip[u + 1]])} for u in range(U)}
    test = {u: t for u, t in test.items() if t}
    cfg = default_config(top_k=k, cutoffs=[cutoff], simple_metrics=list(NAMES), relevance_threshold=thr)
    data = SimpleNamespace(config=cfg, get_test=lambda: test, get_validation=lambda: None)
    ev = Evaluator(data, SimpleNamespace())
    recs = {u: [(int(it), 0.0) for it in recs_idx[u]] for u in range(U)}      # -1 = empty slot: keeps its rank, never hits
    return ev.eval((recs, recs))[cutoff]["test_results"]


# ---- fragile-user report -------------------------------------------------------------------------------------------------
FRAGILE_MARGIN = 1e-9       # no user of a case may have |gap - bound| <= FRAGILE_MARGIN * bound, the planted tie (gap 0) apart
FRAGILE_F = (1, 10, 63, 65, 200)
FRAGILE_N = (1, 5, 701)


def fragile_seed(F, n):
    return 1000 * F + n


def fragile_case(F, n, seed, k=10, u_start=37, item_offset=1000, n_items=300):
    """Crafted [n, k + 1] lists around the bound F 2^-23 |u| max(|i_k|, |i_k+1|): Gu holds u_start + n + 5 users, Gi only the
    items item_offset .. item_offset + n_items.  Rows 0..2 (when n >= 5) are the three kinds of short list, row 3 an exact tie.
    Returns a dict of host arrays with the expected flags / counts of a NumPy fp64 evaluation and the smallest margin."""
    rs = np.random.RandomState(seed)
    Gu = rs.normal(size=(u_start + n + 5, F)).astype(np.float32)
    Gi = rs.normal(size=(n_items, F)).astype(np.float32)
    idx = np.stack([rs.choice(n_items, size=k + 1, replace=False) for _ in range(n)]).astype(np.int32) + item_offset
    nu = np.sqrt((Gu[u_start:u_start + n].astype(np.float64) ** 2).sum(1))
    ni = np.sqrt((Gi.astype(np.float64) ** 2).sum(1))
    bound = F * 2.0 ** -23 * nu * np.maximum(ni[idx[:, k - 1] - item_offset], ni[idx[:, k] - item_offset])
    val = np.empty((n, k + 1), np.float32)
    val[:, k] = (bound * rs.uniform(-4, 4, size=n)).astype(np.float32)
    val[:, k - 1] = (val[:, k].astype(np.float64) + bound * np.exp(rs.uniform(np.log(0.05), np.log(20), size=n))).astype(np.float32)
    for c in range(k - 2, -1, -1):
        val[:, c] = val[:, c + 1] + np.abs(val[:, c + 1]) + np.float32(1.0)
    short = np.zeros(n, bool)
    tie = np.zeros(n, bool)
    if n >= 5:
        idx[0, k] = -1
        val[1, k] = -np.inf
        idx[2, k - 1] = -1
        short[:3] = True
        val[3, k - 1] = val[3, k]
        tie[3] = True
    gap = val[:, k - 1].astype(np.float64) - val[:, k].astype(np.float64)
    flags = (gap < bound) & ~short
    live = ~short & ~tie
    margin = float(np.min(np.abs(gap[live] - bound[live]) / bound[live])) if live.any() else np.inf
    return dict(Gu=Gu, Gi=Gi, idx=idx, val=val, k=k, u_start=u_start, item_offset=item_offset, flags=flags,
                counts=(int(flags.sum()), int(short.sum())), margin=margin, tie=tie)


# ---- the IDCG selection at the edges of its gain buffer: el_rec_metrics and el_fair_metrics run the same pass ----------------------
REL_COUNTS = (0, 1, 63, 64, 65, 511, 512, 513, 960, 961, 1023, 1024, 1025, 1500, 3000)


def idcg_case(cutoff):
    """One user per relevant count, thr 2.5, fractional float32 ratings with runs of ties (quarter steps, 2.5 itself among them);
    entries below the threshold sit between the relevant ones, and the largest gains fill the last 64 entries of the row."""
    rs = np.random.RandomState(77 + cutoff)
    thr, rws = 2.5, []
    for c in REL_COUNTS:
        tail = min(64, c)
        body = c - tail
        b = np.where(rs.rand(body) < 0.5, np.round(rs.uniform(2.5, 4.0, size=body) * 4) / 4, rs.uniform(2.5, 4.0, size=body))
        t = np.where(rs.rand(tail) < 0.5, np.round(rs.uniform(4.5, 5.0, size=tail) * 8) / 8, rs.uniform(4.5, 5.0, size=tail))
        r = [1.25, 2.0]
        for x in b:
            r.append(x)
            if rs.rand() < 0.34:
                r.append(rs.uniform(0.5, 2.49))
        rws.append(np.concatenate([np.array(r), t]).astype(np.float32))
    deg = np.array([len(r) for r in rws])
    ip = np.zeros(len(rws) + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    ratings = np.concatenate(rws)
    items = np.concatenate([2 * np.arange(d) + 1 for d in deg]).astype(np.int32)        # odd ids; the even ones are in no row
    assert [(r >= np.float32(thr)).sum() for r in rws] == list(REL_COUNTS)
    ld = cutoff
    recs = np.empty((len(rws), ld), np.int32)
    for u, d in enumerate(deg):
        row = items[ip[u]:ip[u + 1]]
        out = 2 * rs.choice(8000, size=ld, replace=False)
        pick = np.concatenate([row[-2:][::-1], rs.permutation(row[:-2])])[:(ld + 1) // 2]
        if cutoff == 1 and u % 2:
            pick = pick[:0]
        mix = np.concatenate([pick, out])[:ld]
        recs[u] = mix if cutoff == 1 else rs.permutation(mix)
    return recs, ip, items, ratings, thr
