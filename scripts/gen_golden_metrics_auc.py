"""Generate tests/golden/metrics_auc_ref.npz by RUNNING THE REFERENCE'S OWN Evaluator (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  The reference's
elliot.evaluation.evaluator.Evaluator is imported from that checkout with simple_metrics [AUC, GAUC, LAUC] and handed a stand-in
data object (identity id maps) and FULL-LENGTH recommendation dicts: per user the items outside the train row by (score desc, index
asc), then the train items (the -inf tail of top_k(where(mask, preds, -inf), k = num_items)).

Fixtures, gen(U, I, thr, val, seed) below (own code): float32 scores quantised to halves (many exact ties, some +0.0 / -0.0 pairs);
train rows of 2-12 items; held-out rows of 1-6 items outside the train row with ratings 1-5; about 1 user in 9 without a held-out
row, about 1 in 6 with a held-out row rated all 1; about 1 user in 8 holds out an item the model has no row for (id >= I); with
`val` a second held-out split, disjoint from train and test.  CASES = (U, I, relevance threshold, validation split).  Per case <tag>:
  <tag>_shape = (U, I), _threshold, _cutoffs
  <tag>_scores float32 [U, I]
  <tag>_train_indptr / _train_indices                                   the binary train CSR
  <tag>_test_indptr / _test_indices / _test_ratings / _test_pos         the held-out CSR and, per entry, the position of the item in
                                                                        the reference's list (-1: not in it)
  <tag>_val_*                                                           the same for the validation split (only with `val`)
  <tag>_values float64 [cutoffs, 3], <tag>_val_values                   the reference's AUC, GAUC, LAUC (test_results / val_results)
Asserted here, because the tests rely on it: some user has no relevant item; some user has a held-out id >= I; some target sits
inside a score tie; no user has neg_num <= 0.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_metrics_auc.py <reference checkout>
"""
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
NAMES = ["AUC", "GAUC", "LAUC"]
# (U, I, relevance threshold, validation split)
CASES = [(120, 97, 0, False), (90, 257, 3, False), (64, 130, 2, True)]
CUTOFFS = [10, 5]
SEED0 = 23


def tag_of(U, I, thr, val):
    return f"u{U}_i{I}_t{str(thr).replace('.', 'p')}" + ("_val" if val else "")


def gen(U, I, val, seed):
    r = np.random.RandomState(seed)
    scores = (np.round(r.normal(scale=1.5, size=(U, I)) * 2) / 2).astype(np.float32)
    scores[r.rand(U, I) < 0.02] = np.float32(-0.0)
    train, test, vald = [], [], []
    for u in range(U):
        tr = set(r.choice(I, size=r.randint(2, 13), replace=False).tolist())
        free = np.array(sorted(set(range(I)) - tr))
        r.shuffle(free)
        held, hv, taken = {}, {}, 0
        if r.randint(9) != 0:
            n = r.randint(1, 7)
            ones = r.randint(6) == 0
            held = {int(i): float(1 if ones else r.randint(1, 6)) for i in free[:n]}
            taken = n
            if r.randint(8) == 0:
                held[I + r.randint(5)] = float(r.randint(3, 6))          # an item the model has no row for
        if val and r.randint(7) != 0:
            n = r.randint(1, 5)
            hv = {int(i): float(r.randint(1, 6)) for i in free[taken:taken + n]}
        train.append(tr)
        test.append(held)
        vald.append(hv)
    return scores, train, test, vald


def csr_of(rows, ratings=False):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    cols, vals = [], []
    for u, row in enumerate(rows):
        items = sorted(row)
        indptr[u + 1] = indptr[u] + len(items)
        cols.extend(items)
        if ratings:
            vals.extend(row[i] for i in items)
    return indptr, np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float32)


def full_lists(scores, train):
    """{user: [(item, score), ...]} of length I: admissible items by (score desc, index asc), then the train items at -inf."""
    U, I = scores.shape
    recs = {}
    for u in range(U):
        adm = [i for i in range(I) if i not in train[u]]
        adm.sort(key=lambda i: (-float(scores[u, i] + np.float32(0)), i))
        recs[u] = [(i, float(scores[u, i])) for i in adm] + [(i, float("-inf")) for i in sorted(train[u])]
    return recs


def run_reference(Evaluator, U, I, thr, train, test, vald, recs):
    ids = {i: i for i in range(I)}
    uids = {u: u for u in range(U)}
    indptr, cols, _ = csr_of(train)
    m = sp.csr_matrix((np.ones(cols.shape[0], np.float32), cols, indptr), shape=(U, I))
    ev = SimpleNamespace(cutoffs=list(CUTOFFS), relevance_threshold=thr, paired_ttest=False, simple_metrics=list(NAMES), complex_metrics=[])
    cfg = SimpleNamespace(top_k=I, evaluation=ev, config_test=True)
    test_dict = {u: row for u, row in enumerate(test) if row}
    val_dict = {u: row for u, row in enumerate(vald) if row}
    data = SimpleNamespace(config=cfg, num_users=U, num_items=I, transactions=int(m.nnz), sp_i_train=m, private_items=ids, public_items=ids,
                           private_users=uids, public_users=uids, train_dict={u: {i: 1.0 for i in sorted(row)} for u, row in enumerate(train)},
                           get_test=lambda: test_dict, get_validation=lambda: val_dict or None)
    evaluator = Evaluator(data, SimpleNamespace())
    assert evaluator.get_needed_recommendations() == I
    return evaluator.eval((recs, recs))


def read_positions(recs, rows):
    out = []
    for u, row in enumerate(rows):
        place = {i: n for n, (i, s) in enumerate(recs[u]) if s != float("-inf")}
        out.extend(place.get(i, -1) for i in sorted(row))
    return np.asarray(out, dtype=np.int32)


def main(ref):
    sys.path.insert(0, ref)
    from elliot.evaluation.evaluator import Evaluator
    os.makedirs(OUT, exist_ok=True)
    out, tags = {}, []
    for n_case, (U, I, thr, val) in enumerate(CASES):
        tag = tag_of(U, I, thr, val)
        scores, train, test, vald = gen(U, I, val, SEED0 + n_case)
        recs = full_lists(scores, train)
        res = run_reference(Evaluator, U, I, thr, train, test, vald, recs)
        no_rel = [u for u in range(U) if test[u] and not any(v >= thr for v in test[u].values())]
        assert no_rel or thr == 0, tag
        assert any(not test[u] for u in range(U)), tag
        assert any(i >= I for row in test for i in row), tag
        tied = 0
        for u in range(U):
            for i in test[u]:
                if i < I:
                    tied += int((scores[u] == scores[u, i]).sum() > 1)
            nrel = sum(v >= thr for v in test[u].values())
            assert I - len(train[u]) - nrel + 1 > 0, tag
        assert tied > 0, tag
        qp, qc, _ = csr_of(train)
        out[f"{tag}_shape"] = np.asarray([U, I], np.int64)
        out[f"{tag}_threshold"], out[f"{tag}_cutoffs"] = np.float64(thr), np.asarray(CUTOFFS, np.int64)
        out[f"{tag}_scores"] = scores
        out[f"{tag}_train_indptr"], out[f"{tag}_train_indices"] = qp.astype(np.int32), qc.astype(np.int16)
        for name, rows, key in (("test", test, "test_results"),) + ((("val", vald, "val_results"),) if val else ()):
            tp, tc, tr = csr_of(rows, ratings=True)
            out[f"{tag}_{name}_indptr"], out[f"{tag}_{name}_indices"], out[f"{tag}_{name}_ratings"] = tp.astype(np.int32), tc.astype(np.int16), tr
            out[f"{tag}_{name}_pos"] = read_positions(recs, rows)
            vals = np.asarray([[float(res[c][key][m]) for m in NAMES] for c in CUTOFFS], dtype=np.float64)
            assert np.isfinite(vals).all(), (tag, vals)
            out[f"{tag}_values" if name == "test" else f"{tag}_val_values"] = vals
        tags.append(tag)
        print(f"{tag}: {len(no_rel)} users without a relevant item, {tied} targets inside a tie, test values {out[f'{tag}_values'].tolist()}",
              flush=True)
    assert any(thr > 0 for _, _, thr, _ in CASES)
    out["cases"], out["names"] = np.asarray(tags), np.asarray(NAMES)
    path = os.path.join(OUT, "metrics_auc_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else os.environ["ELLIOT_REF"])
