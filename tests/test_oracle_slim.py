"""The SLIM restatement (tests/helpers/slim_ref.py) against sklearn's own weights and the reference's W (tests/golden/slim_ref.npz,
scripts/gen_golden_slim.py) and, where sklearn is installed, against live ElasticNet fits.  No GPU.

Tolerance rule (columns whose stopping sweep differs from sklearn's): with D_ref = max |W_sklearn32 - W_sklearn64| over the case,
max |W - W_sklearn64| <= max(4 D_ref, 16 * 2^-24 * max |W_sklearn64|) -- two float32 evaluations may each be D_ref from the exact
answer, a different stopping sweep moves an iterate by about as much again; the floor covers a D_ref of a few ulp.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import slim_ref
from tests.helpers.slim_ref import bits, case_matrix, golden_dense, golden_w, load_golden as load

PINNED = ["rat_a0.01_l0.1_n10", "bin_a0.05_l0.5_n20", "rat_a1_l0.01_n10", "ref_a0.001_l0.001_n10", "ref_a0.01_l0.1_n10"]
DEFAULTS = "rat_a0.001_l0.001_n10"
SEED = 42


def case(golden, tag):
    for c in slim_ref.golden_cases(golden):
        if c[0] == tag:
            return c
    raise KeyError(tag)


def test_golden_holds_the_issue_cases(golden):
    z, R = load(golden)
    assert R.shape == (300, 120) and R.nnz == 7947 and int(z["seed"]) == SEED
    assert [c[0] for c in slim_ref.golden_cases(golden)] == PINNED[:3] + [DEFAULTS] + PINNED[3:]
    for tag in PINNED:
        assert z[f"{tag}_same32"].all() and z[f"{tag}_same64"].all(), tag


@pytest.mark.parametrize("tag", PINNED + [DEFAULTS])
def test_restatement_float32_equals_sklearn_and_reference_w(golden, tag):
    """Bit-equal weights before the cut on every column that stops at sklearn's sweep (every column of the pinned cases) and
    the tolerance rule on the rest; W after the cut (the reference's own W_sparse in the ref_ cases) bit for bit."""
    z, R = load(golden)
    _, alpha, l1_ratio, N, exclusion = case(golden, tag)
    I = R.shape[1]
    coef, n_iter = slim_ref.fit(case_matrix(R, tag), alpha, l1_ratio, SEED, exclusion)
    c32, c64 = golden_dense(z, f"{tag}_c32", I, np.float32), golden_dense(z, f"{tag}_c64", I, np.float64)
    same = n_iter == z[f"{tag}_n_iter"]
    assert np.array_equal(same, z[f"{tag}_same32"])
    if tag in PINNED:
        assert same.all()
    assert np.array_equal(bits(coef[same]), bits(c32[same]))
    bound, d_ref = slim_ref.tolerance(c32, c64)
    err = float(np.abs(coef.astype(np.float64) - c64).max())
    print(f"{tag}: same sweep {int(same.sum())}/{I}, D_ref {d_ref:.3g}, bound {bound:.3g}, max err {err:.3g}")
    assert err <= bound
    if same.all():
        W, ties = slim_ref.w_from_coef(coef, N)
        Wg = golden_w(z, tag, I)
        assert ties == 0
        assert np.array_equal(W.indptr, Wg.indptr) and np.array_equal(W.indices, Wg.indices)
        assert np.array_equal(bits(W.data), bits(Wg.data))


@pytest.mark.parametrize("tag", PINNED + [DEFAULTS])
def test_restatement_float64_equals_sklearn(golden, tag):
    z, R = load(golden)
    _, alpha, l1_ratio, N, exclusion = case(golden, tag)
    I = R.shape[1]
    coef, n_iter = slim_ref.fit(case_matrix(R, tag), alpha, l1_ratio, SEED, exclusion, np.float64)
    c32, c64 = golden_dense(z, f"{tag}_c32", I, np.float32), golden_dense(z, f"{tag}_c64", I, np.float64)
    same = n_iter == z[f"{tag}_n_iter64"]
    assert np.array_equal(same, z[f"{tag}_same64"])
    if tag in PINNED:
        assert same.all()
    assert np.array_equal(coef[same], c64[same])
    assert float(np.abs(coef - c64).max()) <= slim_ref.tolerance(c32, c64)[0]


def test_reference_exclusion_is_the_trivial_fit(golden):
    """What `exclusion: reference` reproduces: the target stays among its own regressors, so W[j, j] dominates every column."""
    z, R = load(golden)
    I = R.shape[1]
    c32 = golden_dense(z, "ref_a0.001_l0.001_n10_c32", I, np.float32)
    assert (c32.argmax(1) == np.arange(I)).all()
    assert c32[np.arange(I), np.arange(I)].mean() > 0.99
    assert np.where(np.eye(I, dtype=bool), 0, c32).max() < 0.0075


def test_cut_binds_as_the_generator_found(golden):
    z, R = load(golden)
    I = R.shape[1]
    for tag, alpha, l1_ratio, N, exclusion in slim_ref.golden_cases(golden):
        nnz = (golden_dense(z, f"{tag}_c32", I, np.float32) != 0).sum(1)
        binds = int((nnz - 1 > N).sum())
        W = golden_w(z, tag, I)
        assert np.array_equal(np.diff(W.tocsc().indptr), np.minimum(np.maximum(nnz - 1, 0), N)), tag
        if tag.startswith("bin"):
            assert 0 < binds < I


def live_matrix():
    rs = np.random.RandomState(5)
    R = sp.random(90, 40, density=0.15, random_state=rs, format="csr", dtype=np.float32)
    R.data[:] = rs.randint(1, 6, R.nnz).astype(np.float32)
    return R


@pytest.mark.parametrize("alpha,l1_ratio,exclusion", [(0.02, 0.3, "column"), (0.5, 0.05, "column"), (0.02, 0.3, "reference")])
def test_restatement_against_live_sklearn(alpha, l1_ratio, exclusion):
    pytest.importorskip("sklearn")
    import warnings
    from sklearn.linear_model import ElasticNet
    R = live_matrix()
    X = sp.csc_matrix(R)
    coef, n_iter = slim_ref.fit(R, alpha, l1_ratio, 7, exclusion)
    md = ElasticNet(alpha=alpha, l1_ratio=l1_ratio, positive=True, fit_intercept=False, copy_X=False, precompute=True,
                    selection="random", max_iter=100, random_state=7, tol=1e-4)
    agree = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j in range(R.shape[1]):
            md.fit(slim_ref.masked(X, j, exclusion), X[:, j].toarray())
            if int(np.ravel(md.n_iter_)[0]) == n_iter[j]:
                agree += 1
                assert np.array_equal(bits(np.ravel(md.coef_)), bits(coef[j])), j
    assert agree >= R.shape[1] * 9 // 10


def test_visiting_order_is_sklearns():
    """One sweep with a penalty so large that every visited coordinate is set to 0: started from w = 1 (warm start), the
    coordinates that are still 1 afterwards are exactly those the stream did not draw."""
    pytest.importorskip("sklearn")
    import warnings
    from sklearn.linear_model import ElasticNet
    rs = np.random.RandomState(1)
    I, U = 37, 50
    X = sp.csc_matrix(rs.randint(1, 4, (U, I)).astype(np.float32))
    y = rs.rand(U).astype(np.float32)
    for seed in (0, 42, 123):
        md = ElasticNet(alpha=1e6, l1_ratio=1.0, positive=True, fit_intercept=False, selection="random", max_iter=1,
                        random_state=seed, tol=1e-4, warm_start=True)
        md.coef_ = np.ones(I, np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            md.fit(X, y)
        visited = np.zeros(I, bool)
        visited[slim_ref.order(slim_ref.seed_state(seed), I, I)] = True
        assert not visited.all()                                  # I draws with replacement leave some coordinates out
        assert np.array_equal(np.ravel(md.coef_) == 0, visited), seed


def test_order_wraps_and_handles_a_zero_state():
    o = slim_ref.order(0, 7, 5)
    assert np.array_equal(o, slim_ref.order(1, 7, 5))             # a zero state becomes 1
    s = 1
    for _ in range(3):
        s ^= (s << 13) & 0xffffffff
        s ^= s >> 17
        s ^= (s << 5) & 0xffffffff
    assert o[2] == (s % 2 ** 31) % 7


def test_reference_exclusion_with_more_items_than_users_raises():
    R = sp.random(100, 120, density=0.1, random_state=np.random.RandomState(0), format="csr", dtype=np.float32)
    with pytest.raises(IndexError):
        slim_ref.fit(R, 0.01, 0.1, SEED, "reference")


def test_zero_target_gives_an_empty_list_and_every_sweep():
    R = live_matrix().tolil()
    R[:, 3] = 0
    R = sp.csr_matrix(R)
    coef, n_iter = slim_ref.fit(R, 0.02, 0.3, 7, "column", columns=[3, 4])
    assert not coef[0].any() and n_iter[0] == slim_ref.MAX_ITER and n_iter[1] < slim_ref.MAX_ITER
    idx, val, _ = slim_ref.cut_column(coef[0], 10)
    assert idx.shape == (0,) and val.shape == (0,)
