"""Fixtures of the rank-metric tests (AUC, GAUC, LAUC): the golden cases of scripts/gen_golden_metrics_auc.py as the data object the
stand-alone Evaluator takes, and small CSR helpers for the device tests."""
import os

import numpy as np

from tests.helpers import beyond_ref

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "metrics_auc_ref.npz")
NAMES = ("AUC", "GAUC", "LAUC")
# fp64 sums of at most a few hundred non-negative terms in two orders: <= 2 n 2^-53 relative, far inside the project's bound
TOL = 1e-11


def load():
    return np.load(GOLDEN, allow_pickle=False)


def split_of(z, tag, name):
    if f"{tag}_{name}_indptr" not in z.files:
        return None
    return (z[f"{tag}_{name}_indptr"].astype(np.int64), z[f"{tag}_{name}_indices"].astype(np.int32), z[f"{tag}_{name}_ratings"])


def golden_case(z, tag, metrics, gate=True):
    U, I = (int(v) for v in z[f"{tag}_shape"])
    data = beyond_ref.Data(U, I, (z[f"{tag}_train_indptr"], z[f"{tag}_train_indices"]), split_of(z, tag, "test"), 10,
                           z[f"{tag}_cutoffs"].tolist(), float(z[f"{tag}_threshold"]), metrics, val=split_of(z, tag, "val"))
    if gate:
        data.config.evaluation.rank_metrics = True
    return data


def admissible(z, tag):
    U, I = (int(v) for v in z[f"{tag}_shape"])
    qp, qc = z[f"{tag}_train_indptr"], z[f"{tag}_train_indices"]
    adm = np.ones((U, I), dtype=bool)
    for u in range(U):
        adm[u, qc[qp[u]:qp[u + 1]]] = False
    return adm


def check_values(got, ref_row, what):
    for m, ref in zip(NAMES, ref_row):
        err = abs(got[m] - ref)
        print(f"{what} {m}: {got[m]!r} vs {ref!r}, |diff| {err:.3g}")
        assert err <= TOL * max(1.0, abs(ref)), (what, m, got[m], ref, err)


def csr_of(rows):
    """rows: list of 1-D id arrays (ascending) -> (indptr int64, indices int32)."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rows else np.zeros(0, np.int32)
    return indptr, indices.astype(np.int32)


def mask_of(indptr, indices, n, I, kind):
    """The admissible matrix of a mask CSR: kind "excl" -> everything but the row, "cand" -> the row, None -> everything."""
    if kind is None:
        return None
    adm = np.full((n, I), kind == "excl", dtype=bool)
    for u in range(n):
        row = indices[indptr[u]:indptr[u + 1]]
        adm[u, row[row < I]] = kind == "cand"
    return adm
