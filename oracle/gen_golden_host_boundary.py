"""Generate tests/golden/host_boundary_ref.npz by RUNNING THE REFERENCE'S OWN host framework (build container only).

TEST INFRASTRUCTURE.  Needs the reference checkout on PYTHONPATH (read-only; PYTHONDONTWRITEBYTECODE is forced).  On the
synthetic TSV of write_dataset_tsv() the reference's DataSetLoader + Splitter + DataSet (run.py:59-60) build the data object and
its Evaluator scores the recommendation lists a fixed score table gives under the data object's allunrated_mask
(get_single_recommendation semantics, recommender_utils_mixin.py:84-88).  What is recorded -- ids, split, train matrix, mask,
metric values -- is what tests/test_host_reference_boundary.py holds the package's own data plane, RecMixin, Evaluator mirror
and recommendation writer to.

Run:  PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<elliot checkout> python oracle/gen_golden_host_boundary.py [--out DIR]
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOP_K = 10
CUTOFFS = [10, 5]
METRICS = ["nDCG", "Precision", "Recall"]


def write_dataset_tsv(path):
    """4000 distinct (user, item) rows over 120 users x 300 items, with ratings and timestamps, seeded."""
    rs = np.random.RandomState(0)
    rows = set()
    while len(rows) < 4000:
        rows.add((int(rs.randint(1000, 1120)), int(rs.randint(5000, 5300))))
    with open(path, "w") as f:
        for u, i in sorted(rows):
            f.write(f"{u}\t{i}\t{rs.randint(1, 6)}\t{rs.randint(0, 10**6)}\n")


def stub_scores(U, I):
    """The fixed [U, I] score table the boundary test ranks (the stub model's `_model`)."""
    return np.random.RandomState(7).normal(size=(U, I)).astype(np.float32)


def expected_recs(S, mask, private_users, private_items, k=TOP_K):
    """{public user: [(public item, score)] * k}: the top k of S under the mask, ties by item index."""
    exp = {}
    for u in range(S.shape[0]):
        sc = np.where(mask[u], S[u], -np.inf)
        top = np.argsort(-sc, kind="stable")[:k]
        exp[private_users[u]] = [(private_items[int(i)], float(sc[i])) for i in top]
    return exp


def _triples(d):
    """{user: {item: rating}} -> three arrays in the dict's own order."""
    t = [(u, i, r) for u, its in d.items() for i, r in its.items()]
    return (np.array([x[0] for x in t], np.int64), np.array([x[1] for x in t], np.int64), np.array([x[2] for x in t], np.float64))


def main():
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "tests", "golden")
    import elliot
    from elliot.dataset.dataset import DataSetLoader
    from elliot.evaluation.evaluator import Evaluator
    import elliot.utils.logging as elog

    tmp = tempfile.mkdtemp(prefix="el_host_ref_")
    write_dataset_tsv(os.path.join(tmp, "dataset.tsv"))
    os.makedirs(os.path.join(tmp, "log"), exist_ok=True)
    config = SimpleNamespace(
        config_test=False, binarize=False, random_seed=42, top_k=TOP_K, align_side_with_train=False,
        data_config=SimpleNamespace(strategy="dataset", dataset_path=os.path.join(tmp, "dataset.tsv"), side_information=[]),
        splitting=SimpleNamespace(test_splitting=SimpleNamespace(strategy="random_subsampling", test_ratio=0.2)),
        evaluation=SimpleNamespace(cutoffs=CUTOFFS, simple_metrics=METRICS, relevance_threshold=0, paired_ttest=False,
                                   wilcoxon_test=False, complex_metrics=[]),
        path_log_folder=os.path.join(tmp, "log"))
    elog.init(os.path.join(os.path.dirname(elliot.__file__), "config", "logger_config.yml"), config.path_log_folder)
    data = DataSetLoader(config=config).generate_dataobjects()[0][0]

    pu = [data.private_users[u] for u in range(data.num_users)]
    pi = [data.private_items[i] for i in range(data.num_items)]
    mask = np.asarray(data.allunrated_mask, dtype=bool)
    exp = expected_recs(stub_scores(data.num_users, data.num_items), mask, pu, pi)
    res = Evaluator(data, SimpleNamespace(meta=SimpleNamespace())).eval((exp, exp))
    tr_u, tr_i, tr_r = _triples(data.train_dict)
    te_u, te_i, te_r = _triples({u: v for u, v in data.get_test().items() if v})
    sp = data.sp_i_train.tocsr()
    fx = {
        "users": np.array(list(data.users), np.int64), "items": np.array(list(data.items), np.int64),
        "transactions": np.array([int(data.transactions)], np.int64),
        "private_users": np.array(pu, np.int64), "private_items": np.array(pi, np.int64), "allunrated_mask": mask,
        "train_u": tr_u, "train_i": tr_i, "train_r": tr_r, "test_u": te_u, "test_i": te_i, "test_r": te_r,
        "sp_i_train_indptr": sp.indptr.astype(np.int64), "sp_i_train_indices": sp.indices.astype(np.int64),
        "sp_i_train_data": sp.data.astype(np.float64),
    }
    for c in CUTOFFS:
        for m in METRICS:
            fx[f"ref_{m}@{c}"] = np.array([float(res[c]["test_results"][m])], np.float64)
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "host_boundary_ref.npz"), **fx)
    print("wrote", os.path.join(out_dir, "host_boundary_ref.npz"), {k: v.shape for k, v in fx.items()})


if __name__ == "__main__":
    main()
