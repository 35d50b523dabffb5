"""GPU: el_als_gram / el_als_solve (elliot_amd/csrc/el_als.hip) at the edges of their kernels.  The yardstick of a solve is each row's own
backward error in extended precision (als_ref.backward_error), held to 16 times what the NumPy restatement reaches on the same case
(tests/helpers/als_cases.py; tests/test_als_ref_host.py checks the helper, the cases and the bound without a GPU).
  k_als_solve<T>       F at both ends of T = 16, 64, 256 and the last, partly filled stripe of the packed triangle; 1, NG - 1, NG,
                       NG + 1 rows (dead lane groups); a workgroup whose rows are all long or empty; a row's bits do not depend on
                       where the row stands
  long rows            piece_len - 1, piece_len, piece_len + 1, exact multiples, several long rows, the first and the last row,
                       every row; a plan that does not describe the pattern is reported by row (in-bounds plans only)
  bad pivots           the smallest of two bad rows in different workgroups is named, a NaN pivot counts, the bad rows' X is left
                       alone and every other row is solved
  k_als_gram_part      n = 0, below one LDS tile, at the tile and at the 256-row slot, beyond 512 slots of 256 rows: exact integers
  ops.AlsDeviceState   three steps with long rows on both sides, for both Gram timings
"""
import ctypes as C

import numpy as np
import pytest
import torch

from elliot_amd import ops
from tests.helpers import als_cases as ac
from tests.helpers import als_ref

pytestmark = pytest.mark.gpu

ElliotHipError = ops._lib.ElliotHipError


def dev64(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)


def solve(ctx, indptr, indices, Y, X0, w_A=ac.W_A, skip_empty=False, G=None, n_cols=ac.I, pat=None):
    """One el_als_solve on the pattern from X0: the X it leaves, as NumPy."""
    Yd = dev64(Y, ctx)
    G = ops.als_gram(ctx, Yd) if G is None else G
    pat = ops.AlsCSR(indptr, indices, n_cols, ctx.device, ac.PIECE) if pat is None else pat
    Xd = dev64(X0, ctx)
    ops.als_solve(ctx, pat, Yd, G, w_A, ac.W_B, ac.LAM, Xd, skip_empty=skip_empty)
    return Xd.cpu().numpy()


def check_eta(c, X, rows=None, tag=""):
    """Every row's backward error within the case's bound; prints the largest and its ratio to the restatement's largest."""
    eta = als_ref.backward_error(c.indptr, c.indices, c.Y, getattr(c, "w_A", ac.W_A), ac.W_B, ac.LAM, X, rows=rows)
    ref = c.eta_ref if rows is None else c.eta_ref[rows]
    print("%s F=%d: largest eta %.3g (restatement %.3g, ratio %.3g, bound %.3g)"
          % (tag, c.F, eta.max(), ref.max(), eta.max() / ref.max(), c.bound))
    assert np.all(eta <= c.bound), (tag, c.F, np.flatnonzero(~(eta <= c.bound)), eta.max(), c.bound)


def run_case(ctx, c, tag):
    X = solve(ctx, c.indptr, c.indices, c.Y, c.X0)
    check_eta(c, X, tag=tag)
    assert np.abs(X - c.X_ref).max() <= 1e-12 * np.abs(c.X_ref).max()
    return X


# ---- solve ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ac.SOLVE_F)
def test_solve_at_the_lane_group_edges(ctx, F):
    c = ac.case("shared", F)
    pat = ops.AlsCSR(c.indptr, c.indices, ac.I, ctx.device, ac.PIECE)
    assert (pat.n_long, pat.n_pieces) == ac.plan_counts(c.lens) == (10, 33)
    x1 = run_case(ctx, c, "shared")
    x2 = solve(ctx, c.indptr, c.indices, c.Y, c.X0)
    assert x1.tobytes() == x2.tobytes()
    empty = np.diff(c.indptr) == 0
    assert empty.tolist() == [r in (0, 9) for r in range(c.U)]
    assert np.all(x1[empty] == 0.0)
    xs = solve(ctx, c.indptr, c.indices, c.Y, c.X0, skip_empty=True)
    assert xs[empty].tobytes() == c.X0[empty].tobytes()
    assert xs[~empty].tobytes() == x1[~empty].tobytes()


@pytest.mark.parametrize("F", [16, 17, 65])
def test_a_rows_bits_depend_on_that_row_alone(ctx, F):
    """The rows in reverse order, and behind 13 one-entry rows: other lane groups, other workgroups, other slots, the same bits."""
    c = ac.case("shared", F)
    x1 = solve(ctx, c.indptr, c.indices, c.Y, c.X0)
    rows = [c.indices[c.indptr[r]:c.indptr[r + 1]] for r in range(c.U)]

    def csr(rs):
        return (np.concatenate([[0], np.cumsum([len(r) for r in rs])]).astype(np.int64), np.concatenate(rs).astype(np.int32))
    xr = solve(ctx, *csr(rows[::-1]), c.Y, c.X0[::-1])
    assert xr[::-1].tobytes() == x1.tobytes()
    extra = [np.array([(5 * i) % ac.I], np.int32) for i in range(13)]
    xp = solve(ctx, *csr(extra + rows), c.Y, np.concatenate([np.ones((13, F)), c.X0]))
    assert xp[13:].tobytes() == x1.tobytes()


@pytest.mark.parametrize("F,n", [(F, n) for F, NG in ((8, 16), (20, 4)) for n in (1, NG - 1, NG, NG + 1)])
def test_row_count_edges(ctx, F, n):
    run_case(ctx, ac.case(str(n), F), "%d rows" % n)


def test_a_workgroup_with_no_short_row(ctx):
    c = ac.case("no_short", 8)
    assert all(n == 0 or n > ac.PIECE for n in c.lens[16:32]) and all(0 < n <= ac.PIECE for n in c.lens[:16] + c.lens[32:])
    run_case(ctx, c, "no short row")


@pytest.mark.parametrize("F", [8, 20, 65])
@pytest.mark.parametrize("name", ["long_ends", "all_long"])
def test_long_rows_first_last_and_everywhere(ctx, name, F):
    c = ac.case(name, F)
    pat = ops.AlsCSR(c.indptr, c.indices, ac.I, ctx.device, ac.PIECE)
    assert pat.long_rows.cpu().tolist()[0] == 0 and pat.long_rows.cpu().tolist()[-1] == c.U - 1
    assert (pat.n_long, pat.n_pieces) == ac.plan_counts(c.lens)
    assert name != "all_long" or pat.n_long == c.U
    run_case(ctx, c, name)


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def wrong_plans():
    """The shared case's plan (long rows 4 5 6 7 8 12 14 16 17 18 with 2 2 3 3 6 2 3 3 4 5 pieces), wrong in one way each: (name,
    long_rows, pieces per row, the row the kernels report).  The arrays keep their sizes and every piece number stays below the
    n_pieces the workspace is sized for.
      short_listed  row 3 (16 entries) stands where row 4 (17) should: k_als_piece refuses row 3's two pieces (not a long row),
                    k_als_solve finds row 4 missing; the smaller is reported
      one_too_few   row 12 (17 entries) has one piece: k_als_piece refuses it (2 expected)
      one_too_many  row 6 (33 entries) has four: k_als_piece refuses all four (3 expected; the fourth also starts past the row)"""
    rows = [4, 5, 6, 7, 8, 12, 14, 16, 17, 18]
    pieces = [2, 2, 3, 3, 6, 2, 3, 3, 4, 5]
    yield "short_listed", [3] + rows[1:], pieces, 3
    yield "one_too_few", rows, pieces[:5] + [1] + pieces[6:], 12
    yield "one_too_many", rows, pieces[:2] + [4] + pieces[3:], 6


@pytest.mark.parametrize("F", [8, 20, 65])
def test_plan_mismatch_is_reported_by_row(ctx, F):
    c = ac.case("shared", F)
    good = ops.AlsCSR(c.indptr, c.indices, ac.I, ctx.device, ac.PIECE)
    assert good.long_rows.cpu().tolist() == [4, 5, 6, 7, 8, 12, 14, 16, 17, 18]
    assert np.diff(good.long_first.cpu().numpy()).tolist() == [2, 2, 3, 3, 6, 2, 3, 3, 4, 5]
    for name, rows, pieces, want in wrong_plans():
        pat = ops.AlsCSR(c.indptr, c.indices, ac.I, ctx.device, ac.PIECE)
        first = np.concatenate([[0], np.cumsum(pieces)]).astype(np.int64)
        assert len(rows) == good.n_long and first.shape[0] == good.n_long + 1 and 0 <= min(rows) and max(rows) < c.U
        pat.long_rows = torch.from_numpy(np.asarray(rows, np.int32)).to(ctx.device)
        pat.long_first = torch.from_numpy(first).to(ctx.device)
        pat.n_pieces = int(first[-1])                     # als_solve sizes the workspace by it
        with pytest.raises(ElliotHipError, match=r"does not describe row %d$" % want):
            solve(ctx, c.indptr, c.indices, c.Y, c.X0, pat=pat)
        check_eta(c, solve(ctx, c.indptr, c.indices, c.Y, c.X0, pat=good), tag="after " + name)


def test_pieces_without_a_long_row_are_refused_on_the_host(ctx):
    """n_long = 0 with n_pieces = 1: k_als_piece would search an empty plan and read long_first[1].  Refused before any launch: the
    status words keep what they held."""
    c = ac.case("1", 8)
    F = c.F
    Yd, Xd = dev64(c.Y, ctx), dev64(c.X0, ctx)
    G = ops.als_gram(ctx, Yd)
    pat = ops.AlsCSR(c.indptr, c.indices, ac.I, ctx.device, ac.PIECE)
    long_rows = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    long_first = torch.zeros(2, dtype=torch.int64, device=ctx.device)
    status = torch.full((2,), 12345, dtype=torch.int32, device=ctx.device)
    need = int(ctx.lib.el_als_solve_ws_bytes(1, F))
    ws = torch.zeros(need, dtype=torch.uint8, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx.lib.el_als_solve(ctx.handle, ctx.stream(), p(pat.csr.indptr), p(pat.csr.indices), 1, p(Yd), ac.I, F, p(G), ac.W_A, ac.W_B,
                              ac.LAM, 0, p(long_rows), p(long_first), 0, 1, ac.PIECE, p(Xd), p(status), p(ws), need)
    assert rc != 0
    with pytest.raises(ElliotHipError, match="long-row plan"):
        ops._lib.check(rc, "el_als_solve")
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [12345, 12345]
    assert Xd.cpu().numpy().tobytes() == c.X0.tobytes()
    check_eta(c, solve(ctx, c.indptr, c.indices, c.Y, c.X0), tag="after the refusal")


# ---- bad pivots -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [8, 20])
@pytest.mark.parametrize("kind", ["indefinite", "nan"])
def test_bad_pivots_name_the_smallest_row_and_spare_the_rest(ctx, kind, F):
    c = ac.bad_case(kind, F)
    assert c.bad == [5, 37]
    G = ops.als_gram(ctx, dev64(c.Y, ctx))               # the clean Y's
    Yd, Xd = dev64(c.Y_solve, ctx), dev64(c.X0, ctx)
    assert bool(torch.isnan(Yd).any()) == (kind == "nan")
    pat = ops.AlsCSR(c.indptr, c.indices, ac.BAD_I, ctx.device, ac.PIECE)
    with pytest.raises(np.linalg.LinAlgError, match=r"row 5\b"):
        ops.als_solve(ctx, pat, Yd, G, c.w_A, ac.W_B, ac.LAM, Xd)
    X = Xd.cpu().numpy()
    assert X[c.bad].tobytes() == c.X0[c.bad].tobytes()
    check_eta(c, X, rows=c.good, tag=kind)


# ---- Gram -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(n, F) for F in (1, 17, 128) for n in (0, 1, 31, 32, 33, 255, 256, 257)] + [(131072, 8), (131073, 8)])
def test_gram_edges_exact_on_integers(ctx, n, F):
    """Y in {-2..2}: every partial sum is an integer below 2^53, exact in fp64 in any order.  n = 131073: 511 slots of 257 rows, the
    last of 3."""
    Y = np.random.RandomState(n + F).randint(-2, 3, size=(n, F))
    G = torch.full((F, F), float("nan"), dtype=torch.float64, device=ctx.device)
    ops.als_gram(ctx, dev64(Y, ctx), out=G)
    G = G.cpu().numpy()
    assert np.array_equal(G, Y.T.dot(Y).astype(np.float64))
    assert np.array_equal(G, G.T)
    assert n > 0 or not G.any()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gram", ["fresh", "stale"])
def test_driver_with_long_rows_on_both_sides(ctx, gram):
    U, I, F = 40, 30, 12
    rs = np.random.RandomState(9)
    M = rs.rand(U, I) < 0.3
    M[7, :] = False                                      # one empty user, one empty item
    M[:, 11] = False
    indptr = np.concatenate([[0], np.cumsum(M.sum(axis=1))]).astype(np.int64)
    indices = np.nonzero(M)[1].astype(np.int32)
    X, Y = als_ref.init_tables(4, U, I, F)
    st = ops.AlsDeviceState(ctx, X, Y, indptr, indices, ac.W_A, ac.W_B, ac.LAM, gram=gram, piece_len=4)
    for side, n in ((st.users, U), (st.items, I)):
        assert 0 < side.n_long < n and side.n_pieces > side.n_long and side.empty.sum() == 1
    R, Rt = als_ref.orientations(indptr, indices, U, I)
    step = als_ref.ials_step if gram == "fresh" else als_ref.wrmf_step
    for it in range(3):
        st.step()
        X, Y = step(X, Y, R, Rt, ac.W_A, ac.W_B, ac.LAM)
        for name, got, ref in (("X", st.X, X), ("Y", st.Y, Y)):
            assert np.abs(got.cpu().numpy() - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-300), (gram, name, it)
