"""CPU: the NumPy restatement of EASE^R (tests/helpers/ease_ref.py) against the reference's own EASER.train, recorded in
tests/golden/ease_ref.npz by scripts/gen_golden_ease.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import ease_ref

CASES = ("rat_l5", "rat_l1320", "bin_l50", "cold_item", "empty_user")
WITH_B = ("rat_l5", "rat_l1320", "bin_l50")


def case(g, tag):
    R = sp.csr_matrix((g[f"{tag}_R_data"], g[f"{tag}_R_indices"], g[f"{tag}_R_indptr"]), shape=tuple(g[f"{tag}_shape"]))
    return R, float(g[f"{tag}_l2"])


@pytest.fixture(scope="module")
def g(golden):
    return golden("ease_ref.npz")


@pytest.mark.parametrize("tag", WITH_B)
def test_gram_equals_reference(g, tag):
    """The reference's float32 G, restated: safe_sparse_dot(R.T, R) with the diagonal (float)(n_i + l2_norm)."""
    R, l2 = case(g, tag)
    Gr = (R.T @ R).toarray()                                    # float32 sparse product, as ease_r.py:78
    Gr[np.diag_indices(R.shape[1])] = np.ediff1d(R.tocsc().indptr) + l2
    assert np.array_equal(ease_ref.gram(R, l2), Gr.astype(np.float64))


@pytest.mark.parametrize("tag", WITH_B)
def test_weights_within_reference_float32_error(g, tag):
    R, l2 = case(g, tag)
    B = ease_ref.weights_f64(R, l2)
    Bref = g[f"{tag}_B"]
    assert np.all(np.diag(B) == 0) and np.all(np.diag(Bref) == 0)
    assert np.abs(B.astype(np.float64) - Bref).max() <= 1e-6 * np.abs(Bref).max()


@pytest.mark.parametrize("tag", WITH_B)
def test_reference_scores_are_scipy_product(g, tag):
    """With the reference's B, the restated scores give the reference's recorded lists exactly (values and items)."""
    R, _ = case(g, tag)
    S = ease_ref.scores(R, g[f"{tag}_B"])
    idx, val = ease_ref.topk(S, (R.indptr, R.indices), int(g["k"]))
    ok = ease_ref.same_lists(g[f"{tag}_rec_idx"], idx, S)
    assert ok.all(), np.flatnonzero(~ok)


@pytest.mark.parametrize("tag", CASES)
def test_lists_equal_reference(g, tag):
    R, l2 = case(g, tag)
    S = ease_ref.scores(R, ease_ref.weights_f64(R, l2))
    idx, val = ease_ref.topk(S, (R.indptr, R.indices), int(g["k"]))
    ref_idx = g[f"{tag}_rec_idx"]
    ok = ease_ref.same_lists(ref_idx, idx, S)
    assert ok.all(), np.flatnonzero(~ok)
    if f"{tag}_rec_val" in g:                                    # the reference's own float32 B: agreement to its rounding
        ref_val = g[f"{tag}_rec_val"]
        fin = np.isfinite(ref_val)
        assert np.array_equal(fin, np.isfinite(val))
        assert np.abs(val[fin].astype(np.float64) - ref_val[fin]).max() <= 1e-5 * max(np.abs(ref_val[fin]).max(), 1e-30)


def test_edge_cases_present(g):
    R, _ = case(g, "cold_item")
    assert np.any(np.diff(R.tocsc().indptr) == 0)
    R, _ = case(g, "empty_user")
    assert np.any(np.diff(R.indptr) == 0)


def test_explicit_ratings_make_gram_indefinite(g):
    """Why the device inverse pivots: the reference's G of explicit ratings with a small l2_norm has a negative eigenvalue, so a
    Cholesky factorisation (the ALS kernels' solver) would refuse it; the binary matrix's G is positive definite."""
    R, l2 = case(g, "rat_l5")
    assert np.linalg.eigvalsh(ease_ref.gram(R, l2)).min() < 0
    R, l2 = case(g, "bin_l50")
    assert np.linalg.eigvalsh(ease_ref.gram(R, l2)).min() > 0
