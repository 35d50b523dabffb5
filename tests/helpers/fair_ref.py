"""Fixtures of the fairness metric tests: the golden cases of scripts/gen_golden_metrics_fair.py as the data object, the clustering
files (written where the test says) and the recommendation dicts the stand-alone Evaluator takes; a random label generator for the
device tests."""
import math
import os

import numpy as np

from tests.helpers import beyond_ref

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "metrics_fair_ref.npz")
METRICS = ["RSP", "REO", "BiasDisparityBS", "BiasDisparityBR", "BiasDisparityBD", "UserMADranking", "UserMADrating", "ItemMADranking",
           "ItemMADrating"]


def load():
    return np.load(GOLDEN, allow_pickle=False)


def write_tsv(path, ids, labels):
    with open(path, "w") as f:
        for i, g in zip(ids, labels):
            f.write(f"{int(i)}\t{int(g)}\n")
    return str(path)


def complex_metrics(item_file, user_file, metrics=METRICS, item_name="IG", user_name="UG"):
    """The configuration entries of the reference for the given files (None = no file)."""
    out = []
    for m in metrics:
        if m.startswith("BiasDisparity"):
            d = {"metric": m}
            if item_file:
                d.update(item_clustering_name=item_name, item_clustering_file=item_file)
            if user_file:
                d.update(user_clustering_name=user_name, user_clustering_file=user_file)
        else:
            f, name = (user_file, user_name) if m.startswith("UserMAD") else (item_file, item_name)
            d = {"metric": m, "clustering_name": name}
            if f:
                d["clustering_file"] = f
        out.append(d)
    return out


def label_files(folder, item_labels, user_labels, foreign=()):
    """Writes items.tsv / users.tsv from label arrays (-1 = left out); user_labels None = no user file."""
    keep = np.flatnonzero(item_labels >= 0)
    ids = keep.tolist() + [int(i) for i, _ in foreign]
    labs = item_labels[keep].tolist() + [int(g) for _, g in foreign]
    item_file = write_tsv(os.path.join(str(folder), "items.tsv"), ids, labs)
    user_file = None
    if user_labels is not None:
        keep = np.flatnonzero(user_labels >= 0)
        user_file = write_tsv(os.path.join(str(folder), "users.tsv"), keep.tolist(), user_labels[keep].tolist())
    return item_file, user_file


def golden_case(z, tag, folder, simple=("nDCG",)):
    """(data with complex_metrics configured, lists int32 [U, k], scores float32 [U, k])"""
    U, I, k = (int(v) for v in z[f"{tag}_shape"])
    Gu = int(z[f"{tag}_groups"][1])
    item_file, user_file = label_files(folder, z[f"{tag}_item_labels"].astype(np.int64),
                                       z[f"{tag}_user_labels"].astype(np.int64) if Gu else None, z[f"{tag}_foreign"].tolist())
    data = beyond_ref.Data(U, I, (z[f"{tag}_train_indptr"], z[f"{tag}_train_indices"]),
                           (z[f"{tag}_test_indptr"], z[f"{tag}_test_indices"], z[f"{tag}_test_ratings"]), k, z[f"{tag}_cutoffs"].tolist(),
                           float(z[f"{tag}_threshold"]), list(simple))
    data.config.evaluation.complex_metrics = complex_metrics(item_file, user_file)
    return data, z[f"{tag}_lists"].astype(np.int32), (z[f"{tag}_scores64"].astype(np.float64) / 64.0).astype(np.float32)


def recs_of(lists, scores):
    return {u: [(int(i), float(scores[u, c])) for c, i in enumerate(row) if i >= 0] for u, row in enumerate(lists)}


def check_values(got, names, ref_values, tol, what):
    """got: {name: value} in order; names / ref_values: the reference's.  Same names in the same order, nan where the reference
    has nan, everything else within tol * max(1, |ref|)."""
    assert list(got) == list(names), (what, list(got), list(names))
    for m, ref in zip(names, ref_values):
        v = got[m]
        if math.isnan(ref):
            assert math.isnan(v), (what, m, v)
            continue
        err = abs(v - ref)
        print(f"{what} {m}: {v!r} vs {ref!r}, |diff| {err:.3g}")
        assert err <= tol * max(1.0, abs(ref)), (what, m, v, ref, err)


def random_labels(n, groups, seed, leave_out=15):
    """Labels 0 .. groups-1, each present (n >= groups), about 1 id in `leave_out` without one (-1)."""
    r = np.random.RandomState(seed)
    lab = r.randint(groups, size=n).astype(np.int64)
    out = np.where(r.rand(n) < 1.0 / leave_out, -1, lab)
    out[r.permutation(n)[:groups]] = np.arange(groups)
    return out
