"""The RP3beta restatement (tests/helpers/rp3_ref.py) against the reference's own train() (tests/golden/rp3beta_ref.npz, written
by scripts/gen_golden_rp3beta.py): W bit for bit from the reference's operands, the operands themselves, the lists.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import knn_ref, rp3_ref
from tests.helpers.rp3_ref import bits, case_matrix, golden_cases as tags, golden_operands, load_golden as load, reference_w


def test_fixture_has_seven_cases(golden):
    t = tags(golden)
    assert len(t) == 7
    assert sorted((N, a, b, n) for _, N, a, b, n in t) == sorted(
        [(10, 1., 0.6, False), (10, 0.8, 0.3, True), (20, 1., 0., False)] * 2 + [(-1, 1., 0.6, False)])
    assert sum(tag.startswith("bin") for tag, *_ in t) == 3


def test_restatement_equals_reference_w_and_no_cut_is_tied(golden):
    z, R = load(golden)
    I = R.shape[1]
    for tag, N, alpha, beta, norm in tags(golden):
        Piu, Pui, degree = golden_operands(z, R, tag)
        W, row_ties, col_ties = rp3_ref.build_w(Piu, Pui, degree, N, norm)
        assert (row_ties, col_ties) == (0, 0), tag               # the condition under which the reference's W is comparable
        Wr = reference_w(z, tag, I)
        assert np.array_equal(W.indptr, Wr.indptr) and np.array_equal(W.indices, Wr.indices), tag
        assert np.array_equal(bits(W.data), bits(Wr.data)), tag


def test_restated_operands_without_powers(golden):
    """alpha == 1: Pui and Piu are sums and divisions only (no libm): equal to the reference's bit for bit; beta == 0 likewise."""
    z, R = load(golden)
    for tag, N, alpha, beta, norm in tags(golden):
        if alpha != 1.:
            continue
        Piu, Pui, degree = rp3_ref.operands(case_matrix(R, tag), alpha, beta)
        gPiu, gPui, gdeg = golden_operands(z, R, tag)
        assert np.array_equal(Piu.indices, gPiu.indices) and np.array_equal(Piu.indptr, gPiu.indptr), tag
        assert np.array_equal(bits(Pui.data), bits(gPui.data)) and np.array_equal(bits(Piu.data), bits(gPiu.data)), tag
        if beta == 0.:
            assert np.array_equal(degree, gdeg), tag


def test_restated_operands_with_powers(golden):
    """np.power on float32 (alpha != 1, beta != 0) goes through the host's libm / SIMD kernels: compared where this host
    reproduces the stored values, skipped with that reason where it does not."""
    z, R = load(golden)
    compared = 0
    for tag, N, alpha, beta, norm in tags(golden):
        if alpha == 1. and beta == 0.:
            continue
        Piu, Pui, degree = rp3_ref.operands(case_matrix(R, tag), alpha, beta)
        gPiu, gPui, gdeg = golden_operands(z, R, tag)
        assert Pui.data.dtype == np.float32 and Piu.data.dtype == np.float32 and degree.dtype == np.float64
        if not (np.array_equal(bits(Pui.data), bits(gPui.data)) and np.array_equal(bits(Piu.data), bits(gPiu.data))
                and np.array_equal(degree, gdeg)):
            pytest.skip(f"{tag}: this host's float32 np.power does not reproduce the stored operands (a host libm matter)")
        compared += 1
    assert compared == 5


def test_lists_from_reference_w_equal_reference_lists(golden):
    z, R = load(golden)
    I, k = R.shape[1], int(z["k"])
    users = np.arange(R.shape[0])
    for tag, *_ in tags(golden):
        Rc = case_matrix(R, tag)
        preds = knn_ref.scores(Rc, reference_w(z, tag, I), "item")
        idx, val = knn_ref.topk(preds, users, k, excl=(R.indptr, R.indices))
        ri, rv = z[f"{tag}_rec_idx"], z[f"{tag}_rec_val"]
        assert np.array_equal(bits(val), bits(rv)), tag
        assert knn_ref.cut_ties_equal(idx, val, ri, rv), tag


def test_cuts_bind(golden):
    """The N = 10 cases exercise both cuts: every row of the product holds more than N non-zeros, and the column cut removes
    more than half of what the row cut kept (it binds on the popular columns, 15-29 of them; most columns receive fewer than
    N entries, which is why the reference needs it)."""
    z, R = load(golden)
    I = R.shape[1]
    for tag, N, alpha, beta, norm in tags(golden):
        if N != 10:
            continue
        Piu, Pui, degree = golden_operands(z, R, tag)
        full, _ = rp3_ref.row_lists(Piu, Pui, degree, np.arange(I), I)
        assert sum(len(j) > N for j, _ in full) > I // 2, tag
        lists, _ = rp3_ref.row_lists(Piu, Pui, degree, np.arange(I), N)
        per_col = np.bincount(np.concatenate([j for j, _ in lists]), minlength=I)
        assert (per_col > N).sum() >= 15, tag
        assert np.maximum(per_col - N, 0).sum() > per_col.sum() // 2, tag


def test_row_l1_is_sklearns(golden):
    """The loop el_csr_row_l1 is tested against, pinned to sklearn's normalize(., 'l1') on non-integer values."""
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import normalize
    rs = np.random.RandomState(3)
    X = sp.random(500, 200, density=0.08, random_state=rs, format="csr", dtype=np.float32)
    X.data[:] = rs.uniform(-2.0, 5.0, X.nnz).astype(np.float32)
    X.data[X.indptr[7]:X.indptr[8]] = 0.0                        # a row whose sum is 0 stays as it is
    got = rp3_ref.row_l1(X.indptr, X.data)
    assert np.array_equal(bits(got), bits(normalize(X, norm="l1", axis=1).data))


def test_tie_rules_of_the_restatement():
    """(value desc, index asc) in both cuts, zeros rank between positives and negatives, a float that underflows is dropped
    by the column cut only."""
    keep, tied = rp3_ref._rank_row(np.array([0., 2., 2., 2., 0., -1.]), 0, 2)
    assert keep.tolist() == [1, 2] and tied
    keep, _ = rp3_ref._rank_row(np.array([0., 2., 0., -1., -3.]), 0, 4)       # 1 positive, 2 zeros: one slot left for -1
    assert keep.tolist() == [1, 3]
    idx = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    val = np.array([[1., 0.], [3., 3.], [3., 2.]], np.float32)
    W, tied = rp3_ref.cut(idx, val, np.array([2, 2, 2], np.int32), 3, 1, False)
    assert W.toarray().tolist() == [[0., 0., 0.], [3., 0., 3.], [0., 2., 0.]] and tied == 1      # column 0: rows 1 and 2 tie
    W, tied = rp3_ref.cut(idx, val, np.array([2, 2, 2], np.int32), 3, 2, False)
    assert W.toarray().tolist() == [[0., 1., 0.], [3., 0., 3.], [3., 2., 0.]] and tied == 0 and W.nnz == 5
    Wn, _ = rp3_ref.cut(idx, val, np.array([2, 2, 2], np.int32), 3, 2, True)
    assert np.allclose(Wn.toarray().sum(axis=1), 1.0)
