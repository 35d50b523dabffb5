"""el_slim_order / el_slim_fit / el_slim_w (csrc/el_slim.hip) through ops, against sklearn's own weights and the reference's W
(tests/golden/slim_ref.npz) and the restatement (tests/helpers/slim_ref.py).

The kernel differs from sklearn in the summation order of the dot products and of the gap's scalars only, and therefore sometimes
in the sweep at which a column stops.  Tolerance rule, measured on the reference and never on the kernel: with
D_ref = max |W_sklearn32 - W_sklearn64| over the weights before the cut (the golden's, or the two restatements' where the case is
not in the golden), max |W_gpu - W_sklearn64| <= max(4 D_ref, 16 * 2^-24 * max |W_sklearn64|): two float32 evaluations may each be
D_ref from the exact answer (2 D_ref covers the summation order), a different stopping sweep moves an iterate by about as much
again; the floor covers a D_ref of a few ulp of the largest weight.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.helpers import slim_ref
from tests.helpers.slim_ref import bits, case_matrix, golden_dense, golden_w, load_golden as load

pytestmark = pytest.mark.gpu

GOLDEN_CASES = 6
SEED = 42
LDS_BYTES = 160 * 1024           # SLIM_LDS_BYTES of csrc/el_slim.hip


def golden_case(golden, n):
    z, R = load(golden)
    tag, alpha, l1_ratio, N, exclusion = slim_ref.golden_cases(golden)[n]
    return z, case_matrix(R, tag), tag, alpha, l1_ratio, N, exclusion


def fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion, seed=SEED, j_start=0, j_stop=None, coef=True):
    csc, vals = ops.slim_csc(ctx, R)
    I = R.shape[1]
    order = ops.slim_order(ctx, ops.slim_seed_state(seed), I, ops.SLIM_MAX_ITER * I)
    out = ops.slim_fit(ctx, csc, vals, alpha, l1_ratio, order, N, j_start, j_stop, exclusion=exclusion, coef=coef)
    return [t.cpu().numpy() for t in out]


def rated(indptr, indices, shape, seed):
    rs = np.random.RandomState(seed)
    return sp.csr_matrix((rs.randint(1, 6, indices.shape[0]).astype(np.float32), indices, indptr), shape=shape)


@pytest.mark.parametrize("I", [120, 70001])
def test_order_equals_the_restated_stream(ctx, I):
    from elliot_amd import ops
    n = 2 * I + 5
    for state in (slim_ref.seed_state(SEED), 0, 0xfffffffe):
        got = ops.slim_order(ctx, state, I, n).cpu().numpy()
        assert np.array_equal(got, slim_ref.order(state, I, n)), state


@pytest.mark.parametrize("n", range(GOLDEN_CASES))
def test_weights_within_the_tolerance_rule(ctx, golden, n):
    from elliot_amd import ops
    z, R, tag, alpha, l1_ratio, N, exclusion = golden_case(golden, n)
    I = R.shape[1]
    _, _, _, n_iter, coef = fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion)
    c32, c64 = golden_dense(z, f"{tag}_c32", I, np.float32), golden_dense(z, f"{tag}_c64", I, np.float64)
    bound, d_ref = slim_ref.tolerance(c32, c64)
    err = np.abs(coef.astype(np.float64) - c64).max(1)
    same = n_iter == z[f"{tag}_n_iter"]
    print(f"{tag}: D_ref {d_ref:.3g}, bound {bound:.3g}, max err {err.max():.3g} = {err.max() / d_ref:.2f} D_ref; same sweep as "
          f"sklearn float32 on {int(same.sum())}/{I} columns; bit-equal columns {int((bits(coef) == bits(c32)).all(1).sum())}/{I}; "
          f"columns over the bound {np.flatnonzero(err > bound).tolist()} (their sweeps differ: "
          f"{(~same[err > bound]).tolist()})")
    assert (coef >= 0).all()
    assert err.max() <= bound


@pytest.mark.parametrize("n", range(GOLDEN_CASES))
def test_objective_is_within_sklearns_own_guarantee(ctx, golden, n):
    """F(w_gpu) <= F(w_sklearn32) + tol * y.y per column, F in fp64 on the host: gap < tol * y.y bounds the distance to the optimum."""
    from elliot_amd import ops
    z, R, tag, alpha, l1_ratio, N, exclusion = golden_case(golden, n)
    U, I = R.shape
    coef = fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion)[4]
    c32 = golden_dense(z, f"{tag}_c32", I, np.float32)
    X64 = sp.csc_matrix(R, dtype=np.float64)
    l1, l2 = slim_ref.penalties(alpha, l1_ratio, U)
    worst = -np.inf
    for j in range(I):
        y = X64[:, j].toarray().ravel()
        f_gpu = slim_ref.objective(X64, j, coef[j], l1, l2, exclusion)
        f_ref = slim_ref.objective(X64, j, c32[j], l1, l2, exclusion)
        slack = float(np.float32(slim_ref.TOL)) * float(y @ y)
        worst = max(worst, (f_gpu - f_ref) / slack)
        assert f_gpu <= f_ref + slack, (tag, j, f_gpu, f_ref, slack)
    print(f"{tag}: max (F(w_gpu) - F(w_sklearn32)) / (tol y.y) = {worst:.3g}")


@pytest.mark.parametrize("n", range(GOLDEN_CASES))
def test_cut_equals_the_golden_w(ctx, golden, n):
    """Kept index set per column == the golden's, except FRAGILE columns (last kept and first dropped float32 weight of sklearn
    closer than the bound), at most 5 % of the columns; the kept values within the bound of the golden's."""
    from elliot_amd import ops
    z, R, tag, alpha, l1_ratio, N, exclusion = golden_case(golden, n)
    I = R.shape[1]
    idx, val, cnt, n_iter, coef = fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion)
    c32, c64 = golden_dense(z, f"{tag}_c32", I, np.float32), golden_dense(z, f"{tag}_c64", I, np.float64)
    bound, _ = slim_ref.tolerance(c32, c64)
    Wg = golden_w(z, tag, I).tocsc()
    fragile = 0
    for j in range(I):
        gi, gv = Wg.indices[Wg.indptr[j]:Wg.indptr[j + 1]], Wg.data[Wg.indptr[j]:Wg.indptr[j + 1]]
        ki, kv = idx[j, :cnt[j]], val[j, :cnt[j]]
        assert np.array_equal(bits(kv), bits(coef[j][ki])), j                              # the list holds the weights themselves
        assert (np.diff(kv.astype(np.float64)) <= 0).all(), j                              # in rank order
        if set(ki.tolist()) != set(gi.tolist()):
            srt = np.sort(c32[j][c32[j] != 0])[::-1]
            K = gi.shape[0]
            assert K < srt.shape[0] and srt[K - 1] - srt[K] < bound, (tag, j)              # only a fragile column may differ
            fragile += 1
            continue
        o = np.argsort(ki)
        assert np.array_equal(ki[o], gi) and np.abs(kv[o].astype(np.float64) - gv).max() <= bound, j
    print(f"{tag}: fragile columns {fragile}/{I}")
    assert fragile <= I // 20


def check_w_from_host_lists(ctx, idx, val, cnt):
    from elliot_amd import ops
    I, N = idx.shape
    idx[:, N - 1][cnt < N] = 2 ** 30                                                         # beyond cnt: never read
    W, Wv = ops.slim_w(ctx, *(torch.from_numpy(a).to(ctx.device) for a in (idx, val, cnt)))
    take = np.arange(N)[None, :] < cnt[:, None]
    cols = np.repeat(np.arange(I), cnt)
    E = sp.csr_matrix((val[take], (idx[take], cols)), shape=(I, I), dtype=np.float32)
    E.sort_indices()
    assert np.array_equal(W.indptr.cpu().numpy(), E.indptr)
    assert np.array_equal(W.indices[:W.nnz].cpu().numpy(), E.indices)
    assert np.array_equal(bits(Wv[:W.nnz].cpu().numpy()), bits(E.data))
    return E


def test_w_from_host_lists_is_the_scipy_transpose(ctx):
    rs = np.random.RandomState(3)
    I, N = 3000, 24
    cnt = rs.randint(0, N + 1, I).astype(np.int32)
    cnt[:5] = [0, N, 1, 0, N]
    idx = np.zeros((I, N), np.int32)
    val = rs.uniform(1e-4, 1.0, (I, N)).astype(np.float32)
    pop = 1.0 / np.arange(1, I + 1)
    for j in range(I):
        idx[j, :cnt[j]] = rs.choice(I, cnt[j], replace=False, p=pop / pop.sum())
    check_w_from_host_lists(ctx, idx, val, cnt)


def test_w_from_host_lists_is_the_scipy_transpose_beyond_one_rank_pass(ctx):
    """70 001 targets: one more than the 65 536 one bitmap pass of k_knn_rank covers, so rows of W continue in a second pass at its
    `base` offset.  Row j's columns are start + t * step modulo I: distinct, since N * step < I; the starts favour the low rows,
    and the targets from 65 000 on all start at row 7, whose entries therefore lie on both sides of the pass boundary."""
    rs = np.random.RandomState(4)
    I, N = 70001, 24
    cnt = rs.randint(0, N + 1, I).astype(np.int32)
    cnt[:5] = [0, N, 1, 0, N]
    cnt[[65535, 65536, I - 1]] = N
    start = (I * rs.uniform(0, 1, I) ** 3).astype(np.int64)
    start[65000:] = 7
    step = rs.randint(1, 2001, I)
    idx = ((start[:, None] + step[:, None] * np.arange(N)[None, :]) % I).astype(np.int32)
    idx = np.take_along_axis(idx, rs.uniform(size=(I, N)).argsort(1), 1)                     # the lists are in no column order
    val = rs.uniform(1e-4, 1.0, (I, N)).astype(np.float32)
    assert (np.diff(np.sort(idx, 1), axis=1) > 0).all()
    E = check_w_from_host_lists(ctx, idx, val, cnt)
    row7 = E.indices[E.indptr[7]:E.indptr[8]]
    assert (row7 < 65536).sum() > 256 and (row7 >= 65536).sum() > 256                        # more than one stride of the block, twice


def check_columns(ops, ctx, R, columns, alpha, l1_ratio, exclusion, expect_lds):
    """Single-column calls against the float32 restatement with the float64 restatement as W64."""
    U, I = R.shape
    N = 10
    assert (4 * (U + I) + 64 <= LDS_BYTES) == expect_lds
    csc, vals = ops.slim_csc(ctx, R)
    order = ops.slim_order(ctx, ops.slim_seed_state(SEED), I, ops.SLIM_MAX_ITER * I)
    c32, n32 = slim_ref.fit(R, alpha, l1_ratio, SEED, exclusion, np.float32, columns)
    c64, _ = slim_ref.fit(R, alpha, l1_ratio, SEED, exclusion, np.float64, columns)
    bound, d_ref = slim_ref.tolerance(c32, c64)
    for q, j in enumerate(columns):
        idx, val, cnt, n_iter, coef = (t.cpu().numpy() for t in
                                       ops.slim_fit(ctx, csc, vals, alpha, l1_ratio, order, N, int(j), int(j) + 1,
                                                    exclusion=exclusion, coef=True))
        err = float(np.abs(coef[0].astype(np.float64) - c64[q]).max())
        print(f"U {U} I {I} column {j} (nnz {csc.indptr[j + 1].item() - csc.indptr[j].item()}): sweeps {n_iter[0]} (restatement "
              f"{n32[q]}), err {err:.3g}, D_ref {d_ref:.3g}, bound {bound:.3g}")
        assert err <= bound, j
        ki, kv, _ = slim_ref.cut_column(coef[0], N)
        assert cnt[0] == ki.shape[0] and np.array_equal(idx[0, :cnt[0]], ki) and np.array_equal(bits(val[0, :cnt[0]]), bits(kv))


def spread_columns(R, n=8):
    """n target columns spread over the popularity range, the most and the least popular non-empty ones among them."""
    pop = np.diff(R.tocsc().indptr)
    by_pop = np.argsort(-pop, kind="stable")
    by_pop = by_pop[pop[by_pop] > 0]
    return by_pop[np.linspace(0, by_pop.shape[0] - 1, n).astype(int)]


@pytest.mark.parametrize("exclusion", ["column", "reference"])
def test_global_residual_path(ctx, exclusion):
    """50 000 users: the residual (200 KB) does not fit in LDS and lives in the workspace."""
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    U, I = 50000, 400
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.7, dmin=2, dmax=60, zipf_a=0.9, seed=5)
    R = rated(indptr, indices, (U, I), seed=5)
    check_columns(ops, ctx, R, spread_columns(R), 0.01, 0.1, exclusion, expect_lds=False)


def test_lds_residual_path_at_6040_users(ctx):
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    U, I = 6040, 500
    indptr, indices = zipf_csr(U, I, mean_log=3.0, sigma_log=0.8, dmin=5, dmax=300, zipf_a=0.9, seed=6)
    R = rated(indptr, indices, (U, I), seed=6)
    check_columns(ops, ctx, R, spread_columns(R), 0.01, 0.1, "column", expect_lds=True)


def test_lds_residual_path_near_the_limit(ctx):
    """36 000 users x 400 items: 142 KiB of the 160 KiB a workgroup may declare, still the LDS placement."""
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    U, I = 36000, 400
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.7, dmin=2, dmax=60, zipf_a=0.9, seed=8)
    R = rated(indptr, indices, (U, I), seed=8)
    check_columns(ops, ctx, R, spread_columns(R, 4), 0.01, 0.1, "column", expect_lds=True)


def test_odd_block_equals_the_whole_run_and_is_deterministic(ctx, golden):
    from elliot_amd import ops
    z, R, tag, alpha, l1_ratio, N, exclusion = golden_case(golden, 0)
    full = fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion)
    again = fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion)
    part = fit_all(ops, ctx, R, alpha, l1_ratio, N, exclusion, j_start=37, j_stop=52)
    for a, b, c in zip(full, again, part):
        assert a.tobytes() == b.tobytes()                        # two calls, the same bytes (unused list slots are zero-filled)
        assert a[37:52].tobytes() == c.tobytes()
    W1 = ops.slim_build(ctx, *ops.slim_csc(ctx, R), alpha, l1_ratio, N, SEED, exclusion)
    W2 = ops.slim_build(ctx, *ops.slim_csc(ctx, R), alpha, l1_ratio, N, SEED, exclusion)
    for a, b in zip((W1[0].indptr, W1[0].indices, W1[1], W1[2]), (W2[0].indptr, W2[0].indices, W2[1], W2[2])):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_zero_target_column_and_small_blocks(ctx, golden, monkeypatch):
    """A column without ratings: empty list, every sweep reported; a workspace bound that forces several blocks: the same bytes."""
    from elliot_amd import ops
    z, R, tag, alpha, l1_ratio, N, exclusion = golden_case(golden, 0)
    R = sp.lil_matrix(R)
    R[:, 7] = 0
    R = sp.csr_matrix(R)
    R.eliminate_zeros()
    full = fit_all(ops, ctx, R, alpha, l1_ratio, N, "column")
    idx, val, cnt, n_iter, coef = full
    assert cnt[7] == 0 and n_iter[7] == ops.SLIM_MAX_ITER and not coef[7].any()
    assert (coef[:, 7] == 0).all()                               # and it is nobody's regressor
    assert (n_iter[np.arange(R.shape[1]) != 7] < ops.SLIM_MAX_ITER).all()
    monkeypatch.setattr(ops, "SLIM_FIT_WS_BYTES", 7 * 4 * R.shape[1])
    for a, b in zip(full, fit_all(ops, ctx, R, alpha, l1_ratio, N, "column")):
        assert a.tobytes() == b.tobytes()


def test_error_paths(ctx):
    from elliot_amd import _lib, ops
    rs = np.random.RandomState(0)
    R = sp.random(400, 2100, density=0.01, random_state=rs, format="csr", dtype=np.float32)
    csc, vals = ops.slim_csc(ctx, R)
    order = ops.slim_order(ctx, 1, 2100, ops.SLIM_MAX_ITER * 2100)
    with pytest.raises(_lib.ElliotHipError, match="2048"):
        ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 2049, 0, 4)
    with pytest.raises(_lib.ElliotHipError, match="IndexError"):
        ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 10, 0, 4, exclusion="reference")
    need = int(ctx.lib.el_slim_ws_bytes(400, 2100, 4, 10))
    with pytest.raises(_lib.ElliotHipError, match="workspace too small"):
        ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 10, 0, 4, ws_bytes=need - 256)
    with pytest.raises(ValueError):
        ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 10, 0, 4, exclusion="row")
    idx, val, cnt, n_iter = ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 2048, 0, 4)     # the limit itself is served
    assert idx.shape == (4, 2048)
