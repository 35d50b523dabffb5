"""Generate tests/golden/metrics_fair_ref.npz by RUNNING THE REFERENCE'S OWN Evaluator with complex_metrics (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  The reference's
elliot.evaluation.evaluator.Evaluator is imported from that checkout and handed a stand-in data object (identity id maps),
recommendation dicts and the nine fairness metrics of evaluation/metrics/fairness/ with clustering files written to a temporary
folder; its values are recorded at cutoffs [k, 5].

Fixtures: gen(U, I, k, seed) of scripts/gen_golden_metrics_beyond.py (train / held-out rows and lists), plus, own code below:
scores that are multiples of 2^-6 (exact in fp32, so the reference's doubles are the numbers the device sees), random item and
user labels, clustering files that leave out about 1 id in 15, an item file that also lists two ids outside the catalogue.
CASES = (U, I, k, relevance threshold, item groups, user groups; 0 user groups = no user file, the reference's single-group
branch).  Per case <tag> the file holds
  <tag>_shape = (U, I, k), _threshold, _cutoffs, _groups = (item groups, user groups)
  <tag>_train_indptr / _train_indices, <tag>_test_indptr / _test_indices / _test_ratings     the CSRs
  <tag>_lists int16 [U, k] (-1 pads the end), <tag>_scores64 int16 [U, k] = 64 x the scores
  <tag>_item_labels int8 [I], <tag>_user_labels int8 [U]      -1 = the id is left out of the file
  <tag>_foreign int32 [n, 2]                                  (id, label) rows of the item file outside the catalogue
  <tag>_names, <tag>_values float64 [cutoffs, names]          the reference's result names in its order, and its values
  <tag>_item_counts int64 [cutoffs, 4, Gi]   RSP numerator / denominator, REO numerator / denominator in Python integers
  <tag>_br int64 [cutoffs, Gu, Gi], <tag>_bs int64 [Gu, Gi]   BiasDisparity's count matrices in Python integers
Asserted here, because the tests rely on it: A != R != {} for the thresholds > 0; every RSP / REO denominator and every row sum
of the count matrices is > 0; every value is finite except the MADs over the missing user file; the integer tables reproduce the
reference's P, BR and BS to 1e-12.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_metrics_fair.py <reference checkout>
"""
import math
import os
import sys
import tempfile
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_metrics_beyond import csr_of, gen, tag_of          # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
METRICS = ["RSP", "REO", "BiasDisparityBS", "BiasDisparityBR", "BiasDisparityBD", "UserMADranking", "UserMADrating", "ItemMADranking",
           "ItemMADrating"]
# (U, I, k, relevance threshold, item groups, user groups)
CASES = [(300, 200, 20, 3, 3, 4), (257, 65, 10, 3, 2, 2), (300, 200, 20, 0, 3, 0), (500, 1000, 50, 2.5, 5, 3)]
SEED0 = 11


def labels_of(r, n, groups):
    """Random labels with every group present; about 1 id in 15 left out (-1)."""
    lab = r.randint(groups, size=n)
    lab[r.permutation(n)[:groups]] = np.arange(groups)
    out = lab.copy()
    out[r.rand(n) < 1.0 / 15] = -1
    for g in range(groups):
        assert (out == g).any()
    return out


def write_tsv(path, rows):
    with open(path, "w") as f:
        for i, g in rows:
            f.write(f"{int(i)}\t{int(g)}\n")


def complex_metrics(item_file, user_file):
    out = []
    for m in METRICS:
        if m.startswith("BiasDisparity"):
            d = {"metric": m, "item_clustering_name": "IG", "item_clustering_file": item_file}
            if user_file:
                d.update(user_clustering_name="UG", user_clustering_file=user_file)
        elif m.startswith("UserMAD"):
            d = {"metric": m, "clustering_name": "UG"}
            if user_file:
                d["clustering_file"] = user_file
        else:
            d = {"metric": m, "clustering_name": "IG", "clustering_file": item_file}
        out.append(d)
    return out


def run_reference(Evaluator, U, I, k, thr, cutoffs, train, test, lists, scores, cm):
    ids = {i: i for i in range(I)}
    uids = {u: u for u in range(U)}
    indptr, cols, _ = csr_of(train, I)
    m = sp.csr_matrix((np.ones(cols.shape[0], np.float32), cols, indptr), shape=(U, I))
    ev = SimpleNamespace(cutoffs=list(cutoffs), relevance_threshold=thr, paired_ttest=False, simple_metrics=["nDCG"], complex_metrics=cm)
    cfg = SimpleNamespace(top_k=k, evaluation=ev, config_test=True)
    test_dict = {u: row for u, row in enumerate(test) if row}
    data = SimpleNamespace(config=cfg, num_users=U, num_items=I, transactions=int(m.nnz), sp_i_train=m, private_items=ids, public_items=ids,
                           private_users=uids, public_users=uids, train_dict={u: {i: 1.0 for i in sorted(row)} for u, row in enumerate(train)},
                           get_test=lambda: test_dict, get_validation=lambda: None)
    recs = {u: [(int(i), float(scores[u, c])) for c, i in enumerate(lists[u]) if i >= 0] for u in range(U)}
    res = Evaluator(data, SimpleNamespace()).eval((recs, recs))
    return {c: res[c]["test_results"] for c in cutoffs}


def integer_tables(U, I, thr, cutoff, train, test, lists, ilab, ulab, sizes, Gi, Gu):
    """The numerators / denominators / count matrices in Python integers, straight from the definitions."""
    tab = [[0] * Gi for _ in range(4)]
    br = [[0] * Gi for _ in range(Gu)]
    for u in range(U):
        if not test[u]:
            continue
        lst = [int(i) for i in lists[u][:cutoff] if i >= 0]
        rel = {i for i, v in test[u].items() if v >= thr}
        h = 0 if ulab is None else int(ulab[u])
        for i in lst:
            g = int(ilab[i])
            if g >= 0:
                tab[0][g] += 1
                if h >= 0:
                    br[h][g] += 1
                if i in rel:
                    tab[2][g] += 1
        for g in range(Gi):
            tab[1][g] += sizes[g] - sum(1 for i in train[u] if ilab[i] == g)
        for i in rel - train[u]:
            if ilab[i] >= 0:
                tab[3][int(ilab[i])] += 1
    return tab, br


def main(ref):
    sys.path.insert(0, ref)
    from elliot.evaluation.evaluator import Evaluator
    os.makedirs(OUT, exist_ok=True)
    out, tags = {}, []
    for n_case, (U, I, k, thr, Gi, Gu) in enumerate(CASES):
        tag, cutoffs = tag_of(U, I, k, thr), [k, 5]
        train, test, lists = gen(U, I, k, SEED0 + n_case)
        r = np.random.RandomState(1000 + SEED0 + n_case)
        scores = ((k - np.arange(k))[None, :] * 64 + r.randint(0, 64, size=(U, k)) + r.randint(0, 256, size=(U, 1))) / 64.0
        scores = scores.astype(np.float32)
        assert (scores.astype(np.float64) * 64 == np.round(scores.astype(np.float64) * 64)).all()
        ilab = labels_of(r, I, Gi)
        ulab = labels_of(r, U, Gu) if Gu else None
        foreign = [(I + 5, 0), (I + 9, Gi - 1)]
        A = [u for u in range(U) if test[u]]
        R = [u for u in A if any(v >= thr for v in test[u].values())]
        assert 0 < len(A) < U, tag
        if thr > 0:
            assert 0 < len(R) < len(A), (tag, len(A), len(R))
        with tempfile.TemporaryDirectory() as tmp:
            item_file = os.path.join(tmp, "items.tsv")
            write_tsv(item_file, [(i, g) for i, g in enumerate(ilab) if g >= 0] + foreign)
            user_file = None
            if Gu:
                user_file = os.path.join(tmp, "users.tsv")
                write_tsv(user_file, [(u, g) for u, g in enumerate(ulab) if g >= 0])
            values = run_reference(Evaluator, U, I, k, thr, cutoffs, train, test, lists, scores, complex_metrics(item_file, user_file))
        names = list(values[cutoffs[0]])
        sizes = [int((ilab == g).sum()) + sum(1 for _, fg in foreign if fg == g) for g in range(Gi)]
        n_rows = sum(sizes)
        gu = max(Gu, 1)
        vals = np.zeros((len(cutoffs), len(names)), dtype=np.float64)
        tabs = np.zeros((len(cutoffs), 4, Gi), dtype=np.int64)
        brs = np.zeros((len(cutoffs), gu, Gi), dtype=np.int64)
        bs = [[0] * Gi for _ in range(gu)]
        for u in range(U):
            h = 0 if ulab is None else int(ulab[u])
            if h >= 0:
                for i in train[u]:
                    if ilab[i] >= 0:
                        bs[h][int(ilab[i])] += 1
        iname, uname = "IG", ("UG" if Gu else "")
        for row, c in enumerate(cutoffs):
            assert list(values[c]) == names, tag
            vals[row] = [float(values[c][m]) for m in names]
            for m, v in zip(names, vals[row]):
                assert math.isfinite(v) or (not Gu and m.startswith("UserMAD")), (tag, c, m, v)
            tab, br = integer_tables(U, I, thr, c, train, test, lists, ilab, ulab, sizes, Gi, gu)
            assert all(d > 0 for d in tab[1]) and all(d > 0 for d in tab[3]), (tag, tab)
            assert all(sum(b) > 0 for b in br) and all(sum(b) > 0 for b in bs), (tag, br, bs)
            for g in range(Gi):
                assert abs(tab[0][g] / tab[1][g] - values[c][f"RSP-ProbToBeRanked_items:{iname}-{g}"]) <= 1e-12, (tag, c, g)
                assert abs(tab[2][g] / tab[3][g] - values[c][f"REO-ProbToBeRanked_items:{iname}-{g}"]) <= 1e-12, (tag, c, g)
                for h in range(gu):
                    pc = sizes[g] / n_rows
                    assert abs(br[h][g] / sum(br[h]) / pc - values[c][f"BiasDisparityBR_users:{uname}-{h}_items:{iname}-{g}"]) <= 1e-12
                    assert abs(bs[h][g] / sum(bs[h]) / pc - values[c][f"BiasDisparityBS_users:{uname}-{h}_items:{iname}-{g}"]) <= 1e-12
            tabs[row], brs[row] = tab, br
        tp, tc, tr = csr_of(test, I, ratings=True)
        qp, qc, _ = csr_of(train, I)
        out[f"{tag}_shape"] = np.asarray([U, I, k], np.int64)
        out[f"{tag}_threshold"], out[f"{tag}_cutoffs"] = np.float64(thr), np.asarray(cutoffs, np.int64)
        out[f"{tag}_groups"] = np.asarray([Gi, Gu], np.int64)
        out[f"{tag}_train_indptr"], out[f"{tag}_train_indices"] = qp.astype(np.int32), qc.astype(np.int16)
        out[f"{tag}_test_indptr"], out[f"{tag}_test_indices"], out[f"{tag}_test_ratings"] = tp.astype(np.int32), tc.astype(np.int16), tr
        out[f"{tag}_lists"], out[f"{tag}_scores64"] = lists.astype(np.int16), np.round(scores.astype(np.float64) * 64).astype(np.int16)
        out[f"{tag}_item_labels"] = ilab.astype(np.int8)
        out[f"{tag}_user_labels"] = (ulab if ulab is not None else np.full(U, -1)).astype(np.int8)
        out[f"{tag}_foreign"] = np.asarray(foreign, np.int32)
        out[f"{tag}_names"], out[f"{tag}_values"] = np.asarray(names), vals
        out[f"{tag}_item_counts"], out[f"{tag}_br"], out[f"{tag}_bs"] = tabs, brs, np.asarray(bs, np.int64)
        tags.append(tag)
        print(f"{tag}: |A| {len(A)}, |R| {len(R)}, {len(names)} values per cutoff, item file rows {n_rows}", flush=True)
    out["cases"] = np.asarray(tags)
    path = os.path.join(OUT, "metrics_fair_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else os.environ["ELLIOT_REF"])
