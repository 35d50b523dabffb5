"""GPU: the PureSVD kernels through the C ABI (el_spmm_csr_f64, el_gram_f64, el_psvd_orth, el_psvd_project, el_psvd_signs) and
ops.PureSvdDeviceState.build against the reference's runs in tests/golden/puresvd_ref.npz.

Bounds: the product is compared bit for bit with the documented order; Gram and projection with the standard summation bound
(terms x 2^-53 x the product of the magnitudes); the orthonormalisation with the published Cholesky-QR2 bound
||Q^T Q - I||_F <= 6 (n R + R (R + 1)) 2^-53 (Yamamoto, Nakatsukasa, Yanagisawa & Fukaya 2015); the build with 1 x D, the
reference's own float32-vs-float64 distance (tests/test_oracle_puresvd.py explains why)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.helpers import psvd_ref

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
NONE = 0x7fffffff
CASES = ["u300_i200_f10_s42", "u200_i320_f10_s42", "u400_i250_f32_s42", "u150_i120_f16_s42", "u1000_i600_f50_s42",
         "u600_i900_f100_s42", "u150_i120_f16_s7"]
PIECE = 24                                   # piece length of the product tests: the fixture has rows on both sides of it


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def dev64(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)


def strided(ctx, a, ld):
    """a as the leading columns of a wider device tensor (leading dimension ld), the rest poisoned with NaN."""
    full = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float64, device=ctx.device)
    view = full[:, :a.shape[1]]
    view.copy_(dev64(ctx, a))
    return view


@pytest.fixture(scope="module")
def g(golden):
    return golden("puresvd_ref.npz")


@pytest.fixture(scope="module")
def sparse_fixture():
    """200 x 150, rows of 1 .. 120 entries in shuffled (stored, not sorted) order, one empty row, non-trivial float32 values."""
    rs = np.random.RandomState(5)
    lens = rs.randint(1, 20, 200)
    lens[::9] = rs.randint(PIECE + 1, 121, lens[::9].shape[0])
    lens[7] = 0
    lens[11] = PIECE                           # exactly one piece: still a short row
    lens[13] = 2 * PIECE                       # exactly two pieces
    indptr = np.zeros(201, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate([rs.permutation(150)[:n] for n in lens]).astype(np.int32)
    vals = rs.normal(size=indices.shape[0]).astype(np.float32)
    assert (lens > PIECE).sum() > 5 and (lens <= PIECE).sum() > 5
    return indptr, indices, vals


@pytest.mark.parametrize("R", [11, 20, 60, 110, 256])
@pytest.mark.parametrize("with_vals", [True, False])
def test_spmm_equals_the_documented_order_bit_for_bit(ctx, sparse_fixture, R, with_vals):
    from elliot_amd import ops
    indptr, indices, vals = sparse_fixture
    v = vals if with_vals else None
    X = np.random.RandomState(R).normal(size=(150, R))
    want = psvd_ref.spmm_ordered(indptr, indices, v, X, PIECE)
    A = ops.SpmmCSR(indptr, indices, 150, ctx.device, vals=v, piece_len=PIECE)
    assert A.n_long == int((np.diff(indptr) > PIECE).sum()) and A.n_pieces > A.n_long
    for ldx, ldy in ((R, R), (R + 3, R + 5), (R + 2 + (R & 1), R + 1)):   # contiguous; odd (scalar loads); even (16-byte loads)
        Xd = strided(ctx, X, ldx)
        out = torch.full((200, ldy), float("nan"), dtype=torch.float64, device=ctx.device)[:, :R]
        got = ops.spmm_csr_f64(ctx, A, Xd, out=out).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (R, with_vals, ldx, ldy, np.abs(got - want).max())
        again = ops.spmm_csr_f64(ctx, A, Xd).cpu().numpy()
        assert np.array_equal(bits(again), bits(want))
    one_piece = ops.SpmmCSR(indptr, indices, 150, ctx.device, vals=v, piece_len=1000)      # no long rows at all
    assert one_piece.n_long == 0
    got = ops.spmm_csr_f64(ctx, one_piece, dev64(ctx, X)).cpu().numpy()
    assert np.array_equal(bits(got), bits(psvd_ref.spmm_ordered(indptr, indices, v, X, 1000)))


def test_spmm_reports_a_wrong_plan_and_a_bad_column(ctx, sparse_fixture):
    from elliot_amd import _lib, ops
    indptr, indices, vals = sparse_fixture
    X = dev64(ctx, np.ones((150, 20)))
    A = ops.SpmmCSR(indptr, indices, 150, ctx.device, vals=vals, piece_len=PIECE)
    first_long = int(np.flatnonzero(np.diff(indptr) > PIECE)[0])
    A.long_rows = A.long_rows.clone()
    A.long_rows[0] = first_long + 1                          # a short row where the first long one should be
    with pytest.raises(_lib.ElliotHipError, match=f"plan does not describe row {first_long}"):
        ops.spmm_csr_f64(ctx, A, X)
    bad = indices.copy()
    row = 40
    bad[indptr[row]] = 150                                   # one past the last column
    B = ops.SpmmCSR(indptr, bad, 150, ctx.device, vals=vals, piece_len=PIECE)
    with pytest.raises(_lib.ElliotHipError, match=f"row {row} holds a column index"):
        ops.spmm_csr_f64(ctx, B, X)


@pytest.mark.parametrize("n", [700, 5000])
@pytest.mark.parametrize("R", [20, 110, 150, 256])
def test_gram_is_symmetric_reproducible_and_within_the_summation_bound(ctx, n, R):
    from elliot_amd import ops
    slots = int(ctx.lib.el_gram_f64_slots(n))
    assert (slots == 1) == (n <= 1024)
    Y = np.random.RandomState(n + R).normal(size=(n, R)) * np.linspace(0.1, 3.0, R)[None, :]
    Yd = strided(ctx, Y, R + 3)
    G = ops.gram_f64(ctx, Yd).cpu().numpy()
    assert np.array_equal(bits(G), bits(G.T))
    assert np.array_equal(bits(ops.gram_f64(ctx, Yd).cpu().numpy()), bits(G))
    assert np.array_equal(bits(ops.gram_f64(ctx, dev64(ctx, Y)).cpu().numpy()), bits(G))      # the leading dimension changes nothing
    bound = n * U53 * (np.abs(Y).T @ np.abs(Y))
    err = np.abs(G - Y.T @ Y)
    print(f"gram n={n} R={R} slots={slots}: max error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()


def asymmetric_gram_probe(ctx):
    """Exact small integers with a different pattern in every column: a swapped row / column map cannot pass."""
    from elliot_amd import ops
    rs = np.random.RandomState(0)
    Y = rs.randint(-3, 4, size=(300, 70)).astype(np.float64)
    Y[:, 5] = 0.0
    Y[:, 64:] *= 2.0
    return np.array_equal(ops.gram_f64(ctx, dev64(ctx, Y)).cpu().numpy(), Y.T @ Y)


def test_gram_is_exact_on_small_integers(ctx):
    assert asymmetric_gram_probe(ctx)


def check_orth(ctx, Y, label):
    """el_psvd_orth on Y against the Cholesky-QR2 bound, the span residual and a second run's bits."""
    from elliot_amd import ops
    n, R = Y.shape
    Qd = strided(ctx, Y, R + 1)
    status = ops.psvd_orth(ctx, Qd)
    assert int(status.item()) == NONE
    Q = Qd.cpu().numpy()
    bound = 6.0 * (n * R + R * (R + 1)) * U53
    orth_err = np.linalg.norm(Q.T @ Q - np.eye(R))
    # the span: Y = Q S + E.  (I - Q Q^T) Y = (I - Q Q^T) E + Q (I - Q^T Q) S, so its norm is at most ||E|| + (1 + bound) bound ||Y||;
    # E is the backward error of two products with an explicitly inverted triangular factor, R-term sums each: at most
    # 2 R 2^-53 cond(Y) ||Y|| to first order.  cond(Y) is the input's, computed here.
    cond = np.linalg.cond(Y)
    span_bound = 2.0 * bound + 2.0 * R * U53 * cond
    resid = np.linalg.norm(Y - Q @ (Q.T @ Y)) / np.linalg.norm(Y)
    print(f"{label}: n={n} R={R} cond(Y)={cond:.3g}: ||Q^T Q - I||_F = {orth_err:.3g} ({orth_err / bound:.3g} of the bound), "
          f"residual {resid:.3g} ({resid / span_bound:.3g} of its bound)")
    assert orth_err <= bound
    assert resid <= span_bound
    again = strided(ctx, Y, R + 1)
    ops.psvd_orth(ctx, again)
    assert np.array_equal(bits(again.cpu().numpy()), bits(Q))


@pytest.mark.parametrize("tag", CASES)
def test_orth_meets_the_cholesky_qr2_bound_and_keeps_the_span(ctx, g, tag):
    A = psvd_ref.csr_of(g, tag)
    U, I = A.shape
    R, _, transposed = psvd_ref.plan(U, I, int(g[f"{tag}_factors"]))
    M = sp.csr_matrix(A.T if transposed else A, dtype=np.float64)
    check_orth(ctx, M @ psvd_ref.start_matrix(M.shape[1], R, int(g[f"{tag}_seed"])), tag)


@pytest.mark.parametrize("R", [75, 140, 150])
def test_orth_on_the_widths_between_the_golden_cases(ctx, R):
    """R = 75, 140 and 150 take the projection's 5-, 9- and 12-tile forms; 140 and 150 the Gram's three column blocks.  The input is
    a Gaussian matrix with graded column scales (condition number in the tens)."""
    Y = np.random.RandomState(R).normal(size=(2500, R)) * np.linspace(0.2, 4.0, R)[None, :]
    check_orth(ctx, Y, f"gaussian R={R}")


def test_orth_flags_a_rank_deficient_input(ctx):
    from elliot_amd import ops
    rs = np.random.RandomState(3)
    for n, R, dup in ((500, 20, 13), (3000, 110, 57)):        # the Cholesky in LDS and in memory
        Y = rs.normal(size=(n, R))
        Y[:, dup] = Y[:, 4]
        Yd = dev64(ctx, Y)
        status = ops.psvd_orth(ctx, Yd)
        torch.cuda.synchronize()
        assert int(status.item()) == dup
        ok = dev64(ctx, rs.normal(size=(n, R)))               # and the next call starts clean
        assert int(ops.psvd_orth(ctx, ok, status=status).item()) == NONE


@pytest.mark.parametrize("n, R, k", [(1000, 20, 10), (777, 60, 50), (500, 75, 70), (300, 110, 110), (400, 140, 130),
                                     (300, 180, 170), (513, 256, 246), (64, 256, 256)])
def test_project_within_the_summation_bound_and_rounded_once(ctx, n, R, k):
    from elliot_amd import ops
    rs = np.random.RandomState(n + R + k)
    Y, W = rs.normal(size=(n, R)), rs.normal(size=(R, k))
    scale = np.where(rs.rand(k) < 0.5, -1.0, 1.0)
    Yd, Wd = strided(ctx, Y, R + 3), dev64(ctx, W)
    T64, T32 = ops.psvd_project(ctx, Yd, Wd, f64=True, f32=True)
    T = T64.cpu().numpy()
    bound = R * U53 * (np.abs(Y) @ np.abs(W))
    err = np.abs(T - Y @ W)
    print(f"project n={n} R={R} k={k}: max error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()
    assert np.array_equal(T32.cpu().numpy().view(np.uint32), T.astype(np.float32).view(np.uint32))
    S64, S32 = ops.psvd_project(ctx, Yd, Wd, col_scale=dev64(ctx, scale), f64=True, f32=True)
    assert np.array_equal(bits(S64.cpu().numpy()), bits(T * scale[None, :]))
    assert np.array_equal(S32.cpu().numpy().view(np.uint32), (T * scale[None, :]).astype(np.float32).view(np.uint32))
    only32 = ops.psvd_project(ctx, Yd, Wd, f64=False, f32=True)
    assert only32[0] is None and np.array_equal(only32[1].cpu().numpy(), T32.cpu().numpy())
    if k == R:                                                # in place: every row is read whole before it is written
        ops.psvd_project(ctx, Yd, Wd, out64=Yd)
        assert np.array_equal(bits(Yd.cpu().numpy()), bits(T))


def test_project_is_exact_on_small_integers(ctx):
    """Asymmetric exact data: a wrong lane map of either operand or of the accumulator cannot pass."""
    from elliot_amd import ops
    rs = np.random.RandomState(1)
    Y = rs.randint(-4, 5, size=(200, 37)).astype(np.float64)
    W = rs.randint(-4, 5, size=(37, 23)).astype(np.float64)
    T, _ = ops.psvd_project(ctx, dev64(ctx, Y), dev64(ctx, W))
    assert np.array_equal(T.cpu().numpy(), Y @ W)


def test_signs_follow_numpys_argmax_rule(ctx):
    from elliot_amd import ops
    rs = np.random.RandomState(2)
    T = rs.normal(size=(2000, 33))
    T[100, 0], T[1900, 0] = -9.0, 9.0                         # equal magnitudes in two blocks: the first row decides
    T[1900, 1], T[100, 1] = -9.0, 9.0
    T[700, 2], T[701, 2] = 9.0, -9.0                          # ... and inside one block
    T[:, 3] = -np.abs(T[:, 3])
    want = psvd_ref.flip_signs(T)
    assert want[0] == -1 and want[1] == 1 and want[2] == 1 and want[3] == -1
    got = ops.psvd_signs(ctx, dev64(ctx, T)).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def built(ctx, g):
    from elliot_amd import ops
    cache = {}

    def get(tag):
        if tag not in cache:
            A = psvd_ref.csr_of(g, tag)
            st = ops.PureSvdDeviceState(ctx, A, int(g[f"{tag}_factors"]), int(g[f"{tag}_seed"]))
            st.build(keep_f64=True)
            cache[tag] = (A, st)
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", CASES)
def test_build_scores_within_the_references_own_error(ctx, g, built, tag):
    A, st = built(tag)
    D, rebuild = float(g[f"{tag}_D"]), float(g[f"{tag}_rebuild_err"])
    P64 = psvd_ref.scores(*psvd_ref.ref64_tables(g, tag, A))
    assert st.user_vec.dtype == torch.float32 and tuple(st.user_vec.shape) == (A.shape[0], st.factors)
    assert st.item_vec.dtype == torch.float32 and tuple(st.item_vec.shape) == (A.shape[1], st.factors)
    u64, i64 = st.user_vec64.cpu().numpy(), st.item_vec64.cpu().numpy()
    u32, i32 = st.user_vec.cpu().numpy(), st.item_vec.cpu().numpy()
    assert np.array_equal(u32, u64.astype(np.float32)) and np.array_equal(i32, i64.astype(np.float32))    # rounded once
    for name, user, item in (("fp64 tables", u64, i64), ("float32 tables", u32, i32)):
        err = float(np.abs(psvd_ref.scores(user, item) - P64).max()) + rebuild
        print(f"{tag}: device {name}: max |P - P_ref64| = {err / D:.4g} D (D = {D:.3g}, of which rebuilding {rebuild / D:.3g} D)")
        assert err <= D, (tag, name, err, D)


@pytest.mark.parametrize("tag", CASES)
def test_build_singular_values_and_signs(ctx, g, built, tag):
    A, st = built(tag)
    s32, s64 = g[f"{tag}_sigma32"], g[f"{tag}_sigma64"]
    mine, ref = float(np.abs(st.sigma - s64).max()), float(np.abs(s32 - s64).max())
    print(f"{tag}: device max |sigma - sigma_ref64| = {mine:.3g} (relative {mine / s64.max():.3g}); the reference's float32 run: {ref:.3g}")
    assert mine <= ref
    user64, _ = psvd_ref.ref64_tables(g, tag, A)
    dots = np.einsum("uc,uc->c", st.user_vec64.cpu().numpy(), user64)
    strong = np.abs(dots) > 0.9
    assert strong.sum() >= 0.9 * dots.size and (dots[strong] > 0).all()


@pytest.mark.parametrize("tag", CASES)
def test_rebuild_gives_the_same_bits(ctx, g, built, tag):
    from elliot_amd import ops
    A, st = built(tag)
    again = ops.PureSvdDeviceState(ctx, A, st.factors, st.seed)
    again.build(keep_f64=True)
    for a, b in ((st.user_vec64, again.user_vec64), (st.item_vec64, again.item_vec64)):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    assert np.array_equal(st.sigma, again.sigma)


def test_another_seed_gives_other_tables(ctx, built):
    (_, a), (_, b) = built("u150_i120_f16_s42"), built("u150_i120_f16_s7")
    assert a.seed != b.seed
    assert not np.array_equal(a.user_vec.cpu().numpy(), b.user_vec.cpu().numpy())


def test_build_lists_equal_the_float64_references(ctx, g, built):
    """The device's own top-10 (el_score_topk on the float32 tables) for every user the reference's float32 rounding does not decide."""
    from elliot_amd import ops
    tag = "u1000_i600_f50_s42"
    A, st = built(tag)
    excl = ops.DeviceCSR(A.indptr, A.indices, A.shape[1], ctx.device)
    idx, val = st.recommend(("excl", excl), 10, 0, A.shape[0])
    idx = idx.cpu().numpy()
    P64 = psvd_ref.scores(*psvd_ref.ref64_tables(g, tag, A))
    weak = psvd_ref.fragile(P64, g[f"{tag}_row_err"], A.indptr, A.indices, 10)
    assert weak.sum() <= 0.02 * A.shape[0]
    ref = g[f"{tag}_top64"].astype(np.int32)
    bad = [u for u in np.flatnonzero(~weak) if not np.array_equal(idx[u], ref[u])]
    assert not bad, bad[:10]


def test_rank_deficient_matrix_is_refused(ctx):
    from elliot_amd import ops
    rs = np.random.RandomState(8)
    base = (rs.rand(12, 90) < 0.3).astype(np.float32)        # rank <= 12 < factors + 10
    A = sp.csr_matrix(base[rs.randint(0, 12, 200)])
    st = ops.PureSvdDeviceState(ctx, A, 10, 42)
    with pytest.raises(ValueError, match=r"column \d+ of 20.*rank"):
        st.build()
