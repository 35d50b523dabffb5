"""Beyond-accuracy metrics of the stand-alone evaluator: coverage, concentration, novelty and popularity bias.

  ItemCoverage, UserCoverage, NumRetrieved     metrics/coverage/{item_coverage,user_coverage,num_retrieved}
  Gini, SEntropy                               metrics/diversity/{gini_index,shannon_entropy}
  EFD, EPC                                     metrics/novelty/{EFD/efd.py,EPC/epc.py}
  ARP, APLT, ACLT, PopREO, PopRSP              metrics/bias/{arp,aplt,aclt,pop_reo,pop_rsp}
  popularity, short head, long tail            popularity_utils/popularity.py

Both routes of the evaluator end in `finish`: the device route hands it the sums of el_beyond_metrics / el_beyond_hist_finish /
el_beyond_entropy (include/elliot_hip.h), the dict route those of `numpy_terms` below, an independent NumPy statement of the same
definitions ("Beyond-accuracy metrics").  Populations: A = users with a non-empty held-out row (evaluator.py:121),
R = users of A with an item rated >= the relevance threshold.
"""
import math

import numpy as np

NAMES = ("ItemCoverage", "UserCoverage", "NumRetrieved", "Gini", "SEntropy", "EFD", "EPC", "ARP", "APLT", "ACLT", "PopREO", "PopRSP")
N_SUMS = 18          # layout of el_beyond_metrics' sums (include/elliot_hip.h)


class ItemTables:
    """Per-item tables of one data set, from the array data plane (sp_i_train, transactions), no per-user loop:
      pop    users that hold the item in train (column count of sp_i_train.astype(bool), popularity.py:25-29)
      order  items by pop descending, ties in private-id order (Python's stable sorted(reverse=True), popularity.py:34)
      head   the short head: items of `order` until transactions * 0.8 - sum pop <= 0, the crossing item included (:37-47)
      efd    -log(pop / sum pop) / log 2; an item without train interactions gets the largest novelty, as efd.py does
      epc    1 - pop / number of train users (1 for an item without train interactions, epc.py)"""

    def __init__(self, sp_i_train, transactions, num_train_users=None, pop_ratio=0.8):
        m = sp_i_train.tocsr()
        self.num_items = int(m.shape[1])
        self.pop = np.bincount(m.indices[m.data != 0], minlength=self.num_items).astype(np.int64)
        self.order = np.argsort(-self.pop, kind="stable")
        cum = np.cumsum(self.pop[self.order])
        limit = transactions * pop_ratio
        # `limit -= pop` never rounds (the differences of a shrinking float and integers are exact), so the walk stops at the
        # first prefix sum that reaches the limit
        crossed = np.flatnonzero(cum >= limit)
        n_head = int(crossed[0]) + 1 if crossed.shape[0] else self.num_items
        self.short_head = self.order[:n_head]
        self.head = np.zeros(self.num_items, dtype=bool)
        self.head[self.short_head] = True
        self.n_head = n_head
        norm = float(self.pop.sum())
        seen = self.pop > 0
        log2 = math.log(2)
        self.efd = np.zeros(self.num_items, dtype=np.float64)
        if seen.any():
            self.efd[seen] = np.array([-math.log(p / norm) / log2 for p in self.pop[seen].tolist()])
            self.efd[~seen] = -math.log(int(self.pop[seen].min()) / norm) / log2
        users = int(m.shape[0]) if num_train_users is None else int(num_train_users)
        self.epc = 1.0 - self.pop / float(users)


def discount(cutoff):
    return np.array([math.log(2) / math.log(r + 2) for r in range(cutoff)])


def _member(keys_sorted, keys):
    """positions of `keys` in the ascending `keys_sorted`, -1 where absent"""
    if keys_sorted.shape[0] == 0:
        return np.full(keys.shape, -1, dtype=np.int64)
    pos = np.minimum(np.searchsorted(keys_sorted, keys), keys_sorted.shape[0] - 1)
    return np.where(keys_sorted[pos] == keys, pos, -1)


def numpy_terms(lists, users, test, threshold, train, tables, cutoff):
    """The raw sums of one (split, cutoff) in NumPy.
      lists  int [n, >= cutoff] private item ids, -1 pads the end;  users  int [n] their private user ids
      test   (indptr, cols, ratings) held-out CSR in private ids, rows = users, cols ascending
      train  (indptr, cols) likewise
    Returns (sums float64[18], hist int64[I], entropy_sum): what the three device passes produce."""
    tp, tc, tr = test
    qp, qc = train
    I = tables.num_items
    users = np.asarray(users, dtype=np.int64)
    L = np.asarray(lists, dtype=np.int64)[:, :cutoff]
    keep = tp[users + 1] > tp[users]                                       # A
    users, L = users[keep], L[keep]
    nA = users.shape[0]
    sums = np.zeros(N_SUMS, dtype=np.float64)
    hist = np.zeros(I, dtype=np.int64)
    if nA == 0:
        return sums, hist, 0.0
    W = int(max(I, tc.max(initial=0) + 1, L.max(initial=0) + 1))
    t_rows = np.repeat(np.arange(tp.shape[0] - 1, dtype=np.int64), np.diff(tp))
    t_keys = t_rows * W + tc
    q_rows = np.repeat(np.arange(qp.shape[0] - 1, dtype=np.int64), np.diff(qp))
    q_keys = q_rows * W + qc
    relv = np.asarray(tr, dtype=np.float64) >= threshold
    inR = np.bincount(t_rows[relv], minlength=tp.shape[0] - 1)[users] > 0

    valid = (L >= 0) & (L < I)
    Lc = np.where(valid, L, 0)
    nu = valid.sum(1)
    safe = np.maximum(nu, 1)
    hist = np.bincount(Lc[valid], minlength=I).astype(np.int64)
    tail = valid & ~tables.head[Lc]
    pos = _member(t_keys, users[:, None] * W + Lc)
    hit = valid & (pos >= 0) & relv[np.maximum(pos, 0)]
    disc = discount(cutoff)
    norm = (valid * disc).sum(1)
    nz = np.where(norm > 0, norm, 1.0)
    efd = (hit * disc * tables.efd[Lc]).sum(1) / nz
    epc = (hit * disc * tables.epc[Lc]).sum(1) / nz

    # PopRSP: what of the head / tail the user's train row leaves
    q_head = np.bincount(q_rows[tables.head[qc]], minlength=qp.shape[0] - 1)
    q_len = np.diff(qp)
    den_h = tables.n_head - q_head[users]
    den_t = (I - tables.n_head) - (q_len[users] - q_head[users])
    # PopREO: the relevant items of the user inside the catalogue and outside the train row, by head / tail
    cand = relv & (tc < I)
    cand[cand] = _member(q_keys, t_keys[cand]) < 0
    tcc = np.where(cand, tc, 0)
    r_h = np.bincount(t_rows[cand & tables.head[tcc]], minlength=tp.shape[0] - 1)[users]
    r_t = np.bincount(t_rows[cand & ~tables.head[tcc]], minlength=tp.shape[0] - 1)[users]

    nt = tail.sum(1)
    sums[0], sums[1], sums[2], sums[3] = nA, inR.sum(), (nu > 0).sum(), nu.sum()
    sums[4] = ((tables.pop[Lc] * valid).sum(1) / safe).sum()
    sums[5] = (nt / safe).sum()
    sums[6] = nt.sum()
    sums[7] = nu[inR].sum()
    sums[8], sums[9] = efd[inR].sum(), epc[inR].sum()
    sums[10], sums[11], sums[12], sums[13] = (nu - nt).sum(), nt.sum(), den_h.sum(), den_t.sum()
    sums[14] = (hit & ~tail)[inR].sum()
    sums[15] = (hit & tail)[inR].sum()
    sums[16], sums[17] = r_h[inR].sum(), r_t[inR].sum()

    # SEntropy in the reference's order: item weights w_i = sum over the lists that hold i of 1 / n_u, then sum_i w_i nov_i
    free = int(hist.sum())
    ent = 0.0
    if free:
        w = np.bincount(Lc[valid], weights=np.broadcast_to((1.0 / safe)[:, None], L.shape)[valid], minlength=I)
        seen = hist > 0
        ent = float((w[seen] * (-np.log(hist[seen] / free) / math.log(2))).sum())
    return sums, hist, ent


def gini_numerator(hist, num_items):
    """(n, free, G): G = sum_j (2 (j + I - n + 1) - I - 1) c_(j) over the n non-zero counts ascending, in exact integers."""
    c = np.sort(np.asarray(hist, dtype=np.int64))
    c = c[c > 0]
    n = int(c.shape[0])
    j = np.arange(n, dtype=np.int64)
    G = int(((2 * (j + num_items - n + 1) - num_items - 1) * c).sum())
    return n, int(c.sum()), G


def finish(names, sums, n_recommended, free, G, entropy_sum, num_items):
    """Metric values from the raw sums.  Deviations from the reference, which divides by zero there: a user whose list is empty adds
    0 to ARP / APLT / SEntropy and is still counted; with a one-item catalogue Gini is 0."""
    nA, nR = float(sums[0]), float(sums[1])

    def ratio_cv(num_h, num_t, den_h, den_t):
        with np.errstate(divide="ignore", invalid="ignore"):
            pr = np.array([num_h, num_t], dtype=np.float64) / np.array([den_h, den_t], dtype=np.float64)
            return float(np.std(pr) / np.mean(pr))

    def over(x, n):
        return float(x / n) if n else float("nan")

    out = {}
    for m in names:
        if m == "ItemCoverage":
            out[m] = int(n_recommended)
        elif m == "UserCoverage":
            out[m] = int(round(float(sums[2])))
        elif m == "NumRetrieved":
            out[m] = over(sums[7], nR)
        elif m == "Gini":
            out[m] = 1 - (G / free) / (num_items - 1) if free and num_items > 1 else 0.0
        elif m == "SEntropy":
            out[m] = over(entropy_sum, nA)
        elif m == "EFD":
            out[m] = over(sums[8], nR)
        elif m == "EPC":
            out[m] = over(sums[9], nR)
        elif m == "ARP":
            out[m] = over(sums[4], nA)
        elif m == "APLT":
            out[m] = over(sums[5], nA)
        elif m == "ACLT":
            out[m] = over(sums[6], nA)
        elif m == "PopRSP":
            out[m] = ratio_cv(*sums[10:14])
        elif m == "PopREO":
            out[m] = ratio_cv(*sums[14:18])
    return out
