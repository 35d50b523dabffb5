"""The ItemKNN / UserKNN restatement (tests/helpers/knn_ref.py) pinned to the reference's own output
(tests/golden/knn_{item,user}_ref.npz, scripts/gen_golden_knn.py): W per column, and scores / top-k given the reference's W."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import knn_ref

CASES = [(side, sim, b) for side in ("item", "user") for sim in ("cosine", "dot") for b in ("rat", "bin")]


def load(golden, side):
    return golden(f"knn_{side}_ref.npz")


def input_matrix(z, binary):
    R = sp.csr_matrix((z["R_data"], z["R_indices"], z["R_indptr"]), shape=tuple(z["shape"]))
    if binary:
        R = R.copy()
        R.data[:] = 1.0
    return R


def ref_w(z, tag):
    n = z[f"{tag}_w_indptr"].shape[0] - 1
    return sp.csc_matrix((z[f"{tag}_w_data"], z[f"{tag}_w_indices"], z[f"{tag}_w_indptr"]), shape=(n, n), dtype=np.float32)


@pytest.mark.parametrize("side,sim,b", CASES)
def test_w_columns_match_reference(golden, side, sim, b):
    z = load(golden, side)
    tag = f"{sim}_{b}"
    R = input_matrix(z, b == "bin")
    N = int(z["n_neighbors"])
    M = knn_ref.targets_matrix(R, side)
    n = M.shape[0]
    lists = knn_ref.column_lists(M, np.arange(n), N, sim)
    wp, wi, wd = z[f"{tag}_w_indptr"], z[f"{tag}_w_indices"], z[f"{tag}_w_data"]
    rtol = 1e-5 if sim == "cosine" else 0.0
    binding = 0
    for c in range(n):
        rx, rv = wi[wp[c]:wp[c + 1]], wd[wp[c]:wp[c + 1]]
        ox, ov = lists[c]
        assert len(rx) == len(ox), c
        binding += len(ox) == N
        order = np.lexsort((rx, -rv.astype(np.float64)))
        rx, rv = rx[order], rv[order]
        if sim == "dot":
            assert np.array_equal(ov, rv), c
        else:
            np.testing.assert_allclose(ov, rv, rtol=rtol, atol=0)
        cut = rv.min()                                  # entries within the tolerance of the cut may differ
        near_o = np.abs(ov - cut) <= rtol * abs(cut)
        near_r = np.abs(rv - cut) <= rtol * abs(cut)
        assert set(ox[~near_o].tolist()) == set(rx[~near_r].tolist()), c
    assert binding > n // 2, "the neighbour cut must bind on most columns"


@pytest.mark.parametrize("side,sim,b", CASES)
def test_scores_and_lists_match_reference_given_its_w(golden, side, sim, b):
    z = load(golden, side)
    tag = f"{sim}_{b}"
    R = input_matrix(z, b == "bin")
    W = ref_w(z, tag).tocsr()
    users = np.arange(R.shape[0])
    preds = knn_ref.scores(R, W, side)
    excl = (R.indptr, R.indices)
    k = int(z["k"])
    idx, val = knn_ref.topk(preds, users, k, excl=excl)
    ri, rv = z[f"{tag}_rec_idx"], z[f"{tag}_rec_val"]
    assert np.array_equal(val.view(np.uint32), rv.view(np.uint32))
    assert knn_ref.cut_ties_equal(idx, val, ri, rv)


def test_restatement_w_layout():
    """W's rows hold the targets whose top-N contain them, columns ascending (W.tocsr() of the reference)."""
    rs = np.random.RandomState(0)
    R = sp.random(40, 30, density=0.2, random_state=rs, format="csr", dtype=np.float32)
    R.data[:] = rs.randint(1, 6, size=R.nnz)
    W = knn_ref.build_w(R, "item", 5, "cosine")
    assert W.shape == (30, 30)
    for x in range(30):
        cols = W.indices[W.indptr[x]:W.indptr[x + 1]]
        assert np.all(np.diff(cols) > 0)
    assert np.all(np.diff(W.tocsc().indptr) <= 5)
