"""Fairness metrics of the stand-alone evaluator (`evaluation.complex_metrics`), the nine classes of the reference's
evaluation/metrics/fairness/:

  RSP, REO                                      rsp/rsp.py, reo/reo.py
  BiasDisparityBS, BiasDisparityBR, BiasDisparityBD      BiasDisparity/*.py
  UserMADranking, UserMADrating, ItemMADranking, ItemMADrating      MAD/*.py

A configuration entry is a dict with the reference's keys: `metric`, and `clustering_name` / `clustering_file` (RSP, REO, the
MADs) or `user_clustering_*` / `item_clustering_*` (BiasDisparity).  A clustering file is tab-separated `id<TAB>label`, labels
0 .. C-1 (the reference indexes arrays with them).

Both routes of the evaluator end in `finish`: the device route hands it the integer tables and group sums of el_fair_metrics /
el_group_sums / el_fair_item_finish (include/elliot_hip.h), the dict route those of `numpy_terms` below, an independent NumPy
statement of the same definitions ("Fairness metrics").  Populations: A = users with a non-empty held-out row
(evaluator.py:121), R = users of A with an item rated >= the relevance threshold.

Without a clustering file the reference's `else` branches are kept as they are: BiasDisparity puts every user / item into one
group 0 with P(C) = 1; RSP, REO and the MADs get an EMPTY mapping, so nothing is ever counted and their values are 0/0 = nan.
"""
import csv
import itertools

import numpy as np

from .beyond import _member, discount

NAMES = ("RSP", "REO", "BiasDisparityBS", "BiasDisparityBR", "BiasDisparityBD", "UserMADranking", "UserMADrating", "ItemMADranking",
         "ItemMADrating")
ITEM_ONLY = ("RSP", "REO", "ItemMADranking", "ItemMADrating")
USER_ONLY = ("UserMADranking", "UserMADrating")
PAIR = ("BiasDisparityBS", "BiasDisparityBR", "BiasDisparityBD")
NEED_SCORES = ("UserMADrating", "ItemMADrating")
MAX_GROUPS = 64          # FAIR_MAXG of el_metrics_fair.hip: the workgroup's LDS table holds 64 x 64 pair counts


class Grouping:
    """One clustering in private ids.
      labels    int32[n], -1 = no label
      n_groups  C
      sizes     int64[C]: rows of the file per label, ids outside the id map included (rsp.py:97 `len(i_set - user_train)`)
      rows      rows of the file (BiasDisparity's P(C) = sizes / rows)"""

    def __init__(self, labels, n_groups, sizes, rows, key):
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.n_groups = int(n_groups)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        self.rows = int(rows)
        self.key = key

    @classmethod
    def everything(cls, n):
        """BiasDisparity without a file: one group that holds everything, P(C) = 1."""
        return cls(np.zeros(n, np.int32), 1, [1], 1, "<all>")

    @classmethod
    def nothing(cls, n):
        """RSP / REO / MAD without a file: the reference's empty mapping -- one group, no member."""
        return cls(np.full(n, -1, np.int32), 1, [0], 0, "<none>")

    @classmethod
    def from_file(cls, path, id_map, n):
        ids, labels = read_clustering(path)
        C = len(set(labels))
        if C == 0 or set(labels) != set(range(C)):
            raise Exception(f"Clustering file {path}: labels must be the integers 0 .. C-1 with each present (found {sorted(set(labels))[:8]}"
                            f"{' ...' if C > 8 else ''})")
        if len(set(ids)) != len(ids):
            raise Exception(f"Clustering file {path}: an id is listed twice")
        if C > MAX_GROUPS:
            raise Exception(f"Clustering file {path}: {C} groups; the fairness kernels keep at most {MAX_GROUPS} user groups and "
                            f"{MAX_GROUPS} item groups")
        out = np.full(n, -1, np.int32)
        for i, g in zip(ids, labels):
            p = id_map.get(i)
            if p is not None and 0 <= p < n:
                out[p] = g
        return cls(out, C, np.bincount(np.asarray(labels, np.int64), minlength=C), len(ids), str(path))


def read_clustering(path):
    """(ids, labels) of a tab-separated clustering file without header; ids as integers where every id is one, else as strings."""
    ids, labels = [], []
    with open(path, newline="") as f:
        for row in csv.reader(f, delimiter="\t"):
            if not row:
                continue
            try:
                lab = float(row[1])
                if lab != int(lab):
                    raise ValueError
            except (IndexError, ValueError):
                raise Exception(f"Clustering file {path}: expected `id<TAB>integer label`, found {row}")
            ids.append(row[0])
            labels.append(int(lab))
    try:
        ids = [int(i) for i in ids]
    except ValueError:
        pass
    return ids, labels


class Spec:
    """One configured metric: its canonical name, the two groupings' display names and the pass that serves it."""

    def __init__(self, metric, item_name, user_name, n_pass):
        self.metric, self.item_name, self.user_name, self.n_pass = metric, item_name, user_name, n_pass


class Plan:
    """The configured complex metrics in order, and the passes (item grouping, user grouping) that serve them: a pass is one
    run of the fairness kernels (or of numpy_terms) per (split, cutoff)."""

    def __init__(self, complex_metrics, data):
        self.specs, self.passes = [], []
        U, I = int(data.num_users), int(data.num_items)
        cache = {}

        def grouping(path, kind, absent):
            if not path:
                path = absent.__name__
                if (kind, path) not in cache:
                    cache[(kind, path)] = absent(U if kind == "user" else I)
            if (kind, path) not in cache:
                cache[(kind, path)] = Grouping.from_file(path, data.public_users if kind == "user" else data.public_items,
                                                         U if kind == "user" else I)
            return cache[(kind, path)]

        wants = []
        for entry in complex_metrics:
            entry = dict(entry) if isinstance(entry, dict) else dict(vars(entry))
            name = str(entry.get("metric", ""))
            metric = next((m for m in NAMES if m.lower() == name.lower()), None)
            if metric is None:
                raise Exception(f"Metric {name} is not available in the stand-alone evaluator (supported complex metrics: {NAMES})")
            if metric in PAIR:
                ig = grouping(entry.get("item_clustering_file"), "item", Grouping.everything)
                ug = grouping(entry.get("user_clustering_file"), "user", Grouping.everything)
                names = (entry.get("item_clustering_name", "") if entry.get("item_clustering_file") else "",
                         entry.get("user_clustering_name", "") if entry.get("user_clustering_file") else "")
            elif metric in ITEM_ONLY:
                ig, ug = grouping(entry.get("clustering_file"), "item", Grouping.nothing), None
                # rsp.py / reo.py read the name only with a file; the MADs read it always
                named = entry.get("clustering_file") or metric.startswith("ItemMAD")
                names = (entry.get("clustering_name", "") if named else "", "")
            else:
                ig, ug = None, grouping(entry.get("clustering_file"), "user", Grouping.nothing)
                names = ("", entry.get("clustering_name", ""))
            wants.append((metric, names, ig, ug))
        pairs = []
        for _, _, ig, ug in wants:
            if ig is not None and ug is not None and (ig, ug) not in pairs:
                pairs.append((ig, ug))
        lone_i = [ig for _, _, ig, ug in wants if ug is None and not any(p[0] is ig for p in pairs)]
        lone_u = [ug for _, _, ig, ug in wants if ig is None and not any(p[1] is ug for p in pairs)]
        lone_i = list(dict.fromkeys(lone_i))
        lone_u = list(dict.fromkeys(lone_u))
        for ig, ug in itertools.zip_longest(lone_i, lone_u):
            pairs.append((ig if ig is not None else Grouping.nothing(I), ug if ug is not None else Grouping.nothing(U)))
        self.passes = pairs
        for metric, names, ig, ug in wants:
            n = next(n for n, p in enumerate(pairs) if (ig is None or p[0] is ig) and (ug is None or p[1] is ug))
            self.specs.append(Spec(metric, names[0], names[1], n))
        self.needs_scores = any(s.metric in NEED_SCORES for s in self.specs)
        self.needs_bs = sorted({s.n_pass for s in self.specs if s.metric in ("BiasDisparityBS", "BiasDisparityBD")})


def bs_counts(train, ig, ug):
    """BiasDisparityBS's count matrix int64[Gu, Gi] over every row of the train CSR (indptr, cols)."""
    qp, qc = train
    rows = np.repeat(np.arange(qp.shape[0] - 1, dtype=np.int64), np.diff(qp))
    h, g = ug.labels[rows].astype(np.int64), ig.labels[qc].astype(np.int64)
    ok = (h >= 0) & (g >= 0)
    return np.bincount(h[ok] * ig.n_groups + g[ok], minlength=ug.n_groups * ig.n_groups).reshape(ug.n_groups, ig.n_groups)


def numpy_terms(lists, scores, users, test, threshold, train, ig, ug, cutoff, num_items):
    """The raw tables of one (pass, split, cutoff) in NumPy.
      lists  int [n, >= cutoff] private item ids, -1 pads the end;  scores  float [n, >= cutoff] or None;  users  int [n]
      test   (indptr, cols, ratings) held-out CSR in private ids, rows = users, cols ascending;  train  (indptr, cols) likewise
    Returns what the device passes produce:
      item_counts int64[4, Gi]  RSP numerator, RSP denominator, REO numerator, REO denominator
      pair        int64[Gu, Gi] BiasDisparityBR's counts
      user_sums   float64[Gu, 4] per user group: sum of nDCG, users of R, sum of the mean list score, users that have one
      item_sums   float64[Gi, 2], item_cnt int64[Gi]   sum of v_i (gain, score) and the labelled items in a list of R"""
    tp, tc, tr = test
    qp, qc = train
    I, Gi, Gu = int(num_items), ig.n_groups, ug.n_groups
    U = tp.shape[0] - 1
    users = np.asarray(users, dtype=np.int64)
    order = np.argsort(users, kind="stable")                 # per-item sums run in ascending user order
    users = users[order]
    L = np.asarray(lists, dtype=np.int64)[order][:, :cutoff]
    S = None if scores is None else np.asarray(scores, dtype=np.float64)[order][:, :cutoff]
    keep = tp[users + 1] > tp[users]                         # A
    users, L = users[keep], L[keep]
    S = None if S is None else S[keep]
    out = {"item_counts": np.zeros((4, Gi), np.int64), "pair": np.zeros((Gu, Gi), np.int64), "user_sums": np.zeros((Gu, 4), np.float64),
           "item_sums": np.zeros((Gi, 2), np.float64), "item_cnt": np.zeros(Gi, np.int64)}
    nA = users.shape[0]
    if nA == 0:
        return out
    W = int(max(I, tc.max(initial=0) + 1, L.max(initial=0) + 1))
    t_rows = np.repeat(np.arange(U, dtype=np.int64), np.diff(tp))
    t_keys = t_rows * W + tc
    q_rows = np.repeat(np.arange(qp.shape[0] - 1, dtype=np.int64), np.diff(qp))
    q_keys = q_rows * W + qc
    ratings = np.asarray(tr, dtype=np.float64)
    relv = ratings >= threshold
    present = np.zeros(U, dtype=bool)
    present[users] = True
    inR = np.bincount(t_rows[relv], minlength=U)[users] > 0
    ilab = ig.labels.astype(np.int64)

    valid = (L >= 0) & (L < I)
    Lc = np.where(valid, L, 0)
    gl = np.where(valid, ilab[Lc], -1)
    pos = _member(t_keys, users[:, None] * W + np.where(L >= 0, L, 0))
    found = (L >= 0) & (pos >= 0) & relv[np.maximum(pos, 0)]
    hit = found & valid

    # RSP over A, REO over R
    out["item_counts"][0] = np.bincount(gl[gl >= 0], minlength=Gi)
    q_lab = ilab[qc]
    m = present[q_rows] & (q_lab >= 0)
    out["item_counts"][1] = nA * ig.sizes - np.bincount(q_lab[m], minlength=Gi)
    out["item_counts"][2] = np.bincount(gl[hit & (gl >= 0)], minlength=Gi)
    cand = relv & (tc < I) & present[t_rows]
    cand[cand] = _member(q_keys, t_keys[cand]) < 0
    t_lab = ilab[np.where(cand, tc, 0)]
    out["item_counts"][3] = np.bincount(t_lab[cand & (t_lab >= 0)], minlength=Gi)

    # BiasDisparityBR over A
    hl = ug.labels.astype(np.int64)[users]
    ok = (hl[:, None] >= 0) & (gl >= 0)
    out["pair"] = np.bincount((hl[:, None] * Gi + gl)[ok], minlength=Gu * Gi).reshape(Gu, Gi)

    # per user over R: nDCG (ndcg.py) and the mean list score
    disc = discount(cutoff)
    gain_e = np.zeros(ratings.shape[0], dtype=np.float64)
    gain_e[relv] = np.array([2 ** (r - threshold + 1) - 1 for r in ratings[relv].tolist()])
    gains = np.where(found, gain_e[np.maximum(pos, 0)], 0.0)
    dcg = gains @ disc
    e = np.flatnonzero(relv)
    by = np.lexsort((-gain_e[e], t_rows[e]))
    rows_s, g_s = t_rows[e][by], gain_e[e][by]
    rank = np.arange(rows_s.shape[0]) - np.searchsorted(rows_s, rows_s)
    top = rank < cutoff
    idcg = np.bincount(rows_s[top], weights=g_s[top] * disc[rank[top]], minlength=U)[users]
    ndcg = np.where(dcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0)
    inG = inR & (hl >= 0)
    out["user_sums"][:, 0] = np.bincount(hl[inG], weights=ndcg[inG], minlength=Gu)
    out["user_sums"][:, 1] = np.bincount(hl[inG], minlength=Gu)
    if S is not None:
        nu = valid.sum(1)
        scored = inG & (nu > 0)
        mean = (np.where(valid, S, 0.0)).sum(1) / np.maximum(nu, 1)
        out["user_sums"][:, 2] = np.bincount(hl[scored], weights=mean[scored], minlength=Gu)
        out["user_sums"][:, 3] = np.bincount(hl[scored], minlength=Gu)

    # per item over the lists of R, hits added in ascending user order
    hist = np.bincount(Lc[valid & inR[:, None]], minlength=I)
    sg = np.bincount(Lc[hit], weights=gains[hit], minlength=I)
    ss = np.bincount(Lc[hit], weights=S[hit], minlength=I) if S is not None else np.zeros(I)
    seen = (hist > 0) & (ilab >= 0)
    out["item_sums"][:, 0] = np.bincount(ilab[seen], weights=sg[seen] / hist[seen], minlength=Gi)
    out["item_sums"][:, 1] = np.bincount(ilab[seen], weights=ss[seen] / hist[seen], minlength=Gi)
    out["item_cnt"] = np.bincount(ilab[seen], minlength=Gi)
    return out


def _mad(sums, counts):
    """Mean absolute difference of the group means over all pairs a < b; nan without a pair, as np.average([])."""
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.asarray(sums, dtype=np.float64) / np.asarray(counts, dtype=np.float64)
    diffs = [abs(avg[a] - avg[b]) for a in range(avg.shape[0]) for b in range(a + 1, avg.shape[0])]
    return float(np.average(diffs)) if diffs else float("nan")


def _bias(counts, ig):
    """((category_sum.T / total_sum).T) / PC of BiasDisparityBR.py:115-117 / BiasDisparityBS.py:116-118"""
    counts = np.asarray(counts, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = ig.sizes.astype(np.float64) / float(ig.rows)
        return ((counts.T / counts.sum(1)).T) / pc


def finish(plan, terms, bs):
    """{name: value} in configuration order, each metric expanded into the reference's names and order.
      terms  one dict per pass (numpy_terms' layout);  bs  {pass: BiasDisparityBS's count matrix}
    A group without a member gives 0/0 = nan, as in the reference."""
    out = {}
    for s in plan.specs:
        t = terms[s.n_pass]
        ig, ug = plan.passes[s.n_pass]
        if s.metric in ("RSP", "REO"):
            r = 0 if s.metric == "RSP" else 2
            with np.errstate(divide="ignore", invalid="ignore"):
                P = t["item_counts"][r].astype(np.float64) / t["item_counts"][r + 1].astype(np.float64)
                for g in range(ig.n_groups):
                    out[f"{s.metric}-ProbToBeRanked_items:{s.item_name}-{g}"] = float(P[g])
                out[f"{s.metric}_items:{s.item_name}"] = float(np.std(P) / np.mean(P))
        elif s.metric in PAIR:
            with np.errstate(divide="ignore", invalid="ignore"):
                if s.metric == "BiasDisparityBR":
                    V = _bias(t["pair"], ig)
                elif s.metric == "BiasDisparityBS":
                    V = _bias(bs[s.n_pass], ig)
                else:
                    BR, BS = _bias(t["pair"], ig), _bias(bs[s.n_pass], ig)
                    V = (BR - BS) / BS
            for h in range(ug.n_groups):
                for g in range(ig.n_groups):
                    out[f"{s.metric}_users:{s.user_name}-{h}_items:{s.item_name}-{g}"] = float(V[h, g])
        elif s.metric == "UserMADranking":
            out[f"UserMADranking_{s.user_name}"] = _mad(t["user_sums"][:, 0], t["user_sums"][:, 1])
        elif s.metric == "UserMADrating":
            out[f"UserMADrating_{s.user_name}"] = _mad(t["user_sums"][:, 2], t["user_sums"][:, 3])
        elif s.metric == "ItemMADranking":
            out[f"ItemMADranking_{s.item_name}"] = _mad(t["item_sums"][:, 0], t["item_cnt"])
        elif s.metric == "ItemMADrating":
            out[f"ItemMADrating_{s.item_name}"] = _mad(t["item_sums"][:, 1], t["item_cnt"])
    return out
