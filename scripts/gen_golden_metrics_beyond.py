"""Generate tests/golden/metrics_beyond_ref.npz by RUNNING THE REFERENCE'S OWN Evaluator (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  The reference's
elliot.evaluation.evaluator.Evaluator is imported from that checkout and handed a stand-in data object (identity id maps) and
recommendation dicts; its twelve beyond-accuracy metrics are recorded at cutoffs [k, 5].

Fixtures, gen(U, I, k, seed) below (own code): Zipf-like item popularity; train rows of 3-24 items, every item at least once in
train; held-out rows of 1-5 items outside the train row with ratings 1-5; about 1 user in 11 without a held-out row, about 1 in 7
with a held-out row rated all 1; lists of k items outside the train row, popularity-biased, with planted hits; about 1 list in 13
shorter than k, none empty.  CASES = (U, I, k, relevance threshold).  Per case <tag> the file holds
  <tag>_shape = (U, I, k), _threshold, _cutoffs, _transactions
  <tag>_train_indptr / _train_indices                 the binary train CSR
  <tag>_test_indptr / _test_indices / _test_ratings   the held-out CSR
  <tag>_lists  int16 [U, k], -1 pads the end
  <tag>_head   the reference's short-head id list, in its order
  <tag>_values float64 [cutoffs, 12]                  the reference's values in the order of `names` (integer metrics exact in float64)
  <tag>_G int64 [cutoffs]                             the Gini numerator sum_j (2 (j + I - n + 1) - I - 1) c_(j) in Python integers
Asserted here, because the tests rely on it: A != R != {} for the thresholds > 0; ItemCoverage < I for at least one (case, cutoff);
the four PopREO and PopRSP denominators are > 0; in at least one case the short-head boundary falls inside a popularity tie;
1 - G / free / (I - 1) reproduces the reference's Gini to 1e-12.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_metrics_beyond.py <reference checkout>
"""
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
NAMES = ["ItemCoverage", "UserCoverage", "NumRetrieved", "Gini", "SEntropy", "EFD", "EPC", "ARP", "APLT", "ACLT", "PopREO", "PopRSP"]
# (U, I, k, relevance threshold)
CASES = [(300, 200, 20, 0), (300, 200, 20, 3), (257, 65, 10, 3), (500, 1000, 50, 2.5)]
SEED0 = 11


def tag_of(U, I, k, thr):
    return f"u{U}_i{I}_k{k}_t{str(thr).replace('.', 'p')}"


def gen(U, I, k, seed):
    r = np.random.RandomState(seed)
    w = (1.0 / np.arange(1, I + 1) ** 0.9)[r.permutation(I)]
    w /= w.sum()
    train = []
    for u in range(U):
        n = min(r.randint(3, 25), I - k - 5)
        train.append(set(r.choice(I, size=n, replace=False, p=w).tolist()))
    seen = set().union(*train)
    for i in range(I):
        if i not in seen:
            train[r.randint(U)].add(i)
    test, lists = [], np.full((U, k), -1, dtype=np.int64)
    for u in range(U):
        free = np.array(sorted(set(range(I)) - train[u]))
        held = {}
        if r.randint(11) != 0:
            items = r.choice(free, size=r.randint(1, 6), replace=False)
            ones = r.randint(7) == 0
            held = {int(i): float(1 if ones else r.randint(1, 6)) for i in items}
        test.append(held)
        p = w[free] / w[free].sum()
        lst = r.choice(free, size=k, replace=False, p=p).tolist()
        for i in held:                                                   # planted hits
            if r.rand() < 0.5 and i not in lst:
                lst[r.randint(k)] = i
        n = r.randint(1, k) if r.randint(13) == 0 else k
        lists[u, :n] = lst[:n]
    return train, test, lists


def csr_of(rows, I, ratings=False):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    cols, vals = [], []
    for u, row in enumerate(rows):
        items = sorted(row)
        indptr[u + 1] = indptr[u] + len(items)
        cols.extend(items)
        if ratings:
            vals.extend(row[i] for i in items)
    return indptr, np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float32)


def run_reference(Evaluator, U, I, k, thr, cutoffs, train, test, lists):
    ids = {i: i for i in range(I)}
    uids = {u: u for u in range(U)}
    indptr, cols, _ = csr_of(train, I)
    m = sp.csr_matrix((np.ones(cols.shape[0], np.float32), cols, indptr), shape=(U, I))
    ev = SimpleNamespace(cutoffs=list(cutoffs), relevance_threshold=thr, paired_ttest=False, simple_metrics=list(NAMES), complex_metrics=[])
    cfg = SimpleNamespace(top_k=k, evaluation=ev, config_test=True)
    test_dict = {u: row for u, row in enumerate(test) if row}
    data = SimpleNamespace(config=cfg, num_users=U, num_items=I, transactions=int(m.nnz), sp_i_train=m, private_items=ids, public_items=ids,
                           private_users=uids, public_users=uids, train_dict={u: {i: 1.0 for i in sorted(row)} for u, row in enumerate(train)},
                           get_test=lambda: test_dict, get_validation=lambda: None)
    recs = {u: [(int(i), float(k - c)) for c, i in enumerate(lists[u]) if i >= 0] for u in range(U)}
    evaluator = Evaluator(data, SimpleNamespace())
    res = evaluator.eval((recs, recs))
    head = list(evaluator._pop.get_short_head())
    pop = evaluator._pop.get_pop_items()
    order = list(evaluator._pop.get_sorted_pop_items().keys())
    tie = len(head) < I and pop[head[-1]] == pop[order[len(head)]]
    return {c: res[c]["test_results"] for c in cutoffs}, head, tie, data


def python_G(lists, test, I, cutoff):
    cnt = {}
    for u, row in enumerate(lists):
        if test[u]:
            for i in row[:cutoff]:
                if i >= 0:
                    cnt[int(i)] = cnt.get(int(i), 0) + 1
    n, free = len(cnt), sum(cnt.values())
    return sum((2 * (j + I - n + 1) - I - 1) * c for j, c in enumerate(sorted(cnt.values()))), free, n


def main(ref):
    sys.path.insert(0, ref)
    from elliot.evaluation.evaluator import Evaluator
    os.makedirs(OUT, exist_ok=True)
    out, tags, ties, uncovered = {}, [], 0, 0
    for n_case, (U, I, k, thr) in enumerate(CASES):
        tag, cutoffs = tag_of(U, I, k, thr), [k, 5]
        train, test, lists = gen(U, I, k, SEED0 + n_case)
        assert all(3 <= len(t) for t in train) and set().union(*train) == set(range(I)), tag
        assert (lists[:, 0] >= 0).all() and ((lists >= 0).sum(1) < k).any(), tag
        values, head, tie, data = run_reference(Evaluator, U, I, k, thr, cutoffs, train, test, lists)
        A = [u for u in range(U) if test[u]]
        R = [u for u in A if any(v >= thr for v in test[u].values())]
        assert 0 < len(A) < U, tag
        if thr > 0:
            assert 0 < len(R) < len(A), (tag, len(A), len(R))
        hs = set(head)
        den = np.zeros(4, dtype=np.int64)
        for u in A:
            den[0] += len(hs - train[u])
            den[1] += I - len(hs) - len(train[u] - hs)
        for u in R:
            rel = {i for i, v in test[u].items() if v >= thr} - train[u]
            den[2] += len(rel & hs)
            den[3] += len(rel - hs)
        assert (den > 0).all(), (tag, den)
        ties += int(tie)
        vals = np.zeros((len(cutoffs), len(NAMES)), dtype=np.float64)
        Gs = np.zeros(len(cutoffs), dtype=np.int64)
        for r, c in enumerate(cutoffs):
            assert set(values[c]) == set(NAMES), (tag, sorted(values[c]))
            vals[r] = [float(values[c][m]) for m in NAMES]
            assert np.isfinite(vals[r]).all(), (tag, c, vals[r])
            G, free, n = python_G(lists, test, I, c)
            assert n == values[c]["ItemCoverage"], tag
            assert abs((1 - G / free / (I - 1)) - values[c]["Gini"]) <= 1e-12, (tag, c)
            uncovered += int(n < I)
            Gs[r] = G
        tp, tc, tr = csr_of(test, I, ratings=True)
        qp, qc, _ = csr_of(train, I)
        out[f"{tag}_shape"] = np.asarray([U, I, k], np.int64)
        out[f"{tag}_threshold"], out[f"{tag}_cutoffs"] = np.float64(thr), np.asarray(cutoffs, np.int64)
        out[f"{tag}_transactions"] = np.int64(data.transactions)
        out[f"{tag}_train_indptr"], out[f"{tag}_train_indices"] = qp.astype(np.int32), qc.astype(np.int16)
        out[f"{tag}_test_indptr"], out[f"{tag}_test_indices"], out[f"{tag}_test_ratings"] = tp.astype(np.int32), tc.astype(np.int16), tr
        out[f"{tag}_lists"] = lists.astype(np.int16)
        out[f"{tag}_head"] = np.asarray(head, np.int32)
        out[f"{tag}_values"], out[f"{tag}_G"] = vals, Gs
        tags.append(tag)
        print(f"{tag}: |A| {len(A)}, |R| {len(R)}, head {len(head)} of {I}, boundary in a tie: {bool(tie)}, denominators {den.tolist()}, "
              f"ItemCoverage {[int(v) for v in vals[:, 0]]}", flush=True)
    assert ties >= 1, "no case has its short-head boundary inside a popularity tie: pick another SEED0"
    assert uncovered >= 1, "every (case, cutoff) covers the whole catalogue"
    out["cases"], out["names"] = np.asarray(tags), np.asarray(NAMES)
    path = os.path.join(OUT, "metrics_beyond_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else os.environ["ELLIOT_REF"])
