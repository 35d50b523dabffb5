"""GPU: the shared row scorer and tile transpose (elliot_amd/csrc/el_rowscore.h) at their edges, through ops.csr_dense_scores,
ops.slope_scores, ops.bprslim_scores, ops.slope_table and ops.bprslim_table, bit for bit.

The reference is a NumPy chain that is exact by construction: per entry of the row, in stored order, one rounded elementwise add
of a table row on float64 arrays (EASE^R: one rounded product and one rounded add on float32 arrays), which is what the kernel
does per target.  Catalogue sizes cover every lane stride q of a slab (256 targets each), the slab border and a last slab one
column wide; users [2, 7) of a 7-user CSR have rows of length 0, 1, 2, 70 and one with a repeated column.  Tables and outputs
have leading dimensions wider than I; the cells beyond I hold sentinels that no result may depend on and no store may touch."""
import numpy as np
import pytest
import torch

from elliot_amd import ops

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 1281, 2049]
PAD = 3                     # cells behind I in every row of a table or an output
SENTINEL = -7.25
POISON = 1e300              # what the guard cells of a table hold: a sum that met one is far from its reference
U_START, U_STOP = 2, 7
QNAN = np.uint64(0x7ff8000000000000)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def rows_for(I, seed):
    """(indptr, indices) of 7 users; users 2..6: no entry, 1, 2, 70 (first and last column among them) and a, b, a, c, a."""
    rs = np.random.RandomState(seed)
    a, b, c = rs.randint(0, I, 3)
    long = rs.randint(0, I, 70)
    long[:2] = 0, I - 1
    rows = [rs.randint(0, I, 3), rs.randint(0, I, 3), np.zeros(0, int), rs.randint(0, I, 1), rs.randint(0, I, 2), long,
            np.array([a, b, a, c, a])]
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32)


def padded(ctx, M, fill):
    """(device view [rows, I] with row stride I + PAD, its whole buffer) of a host matrix; the cells behind I hold `fill`."""
    buf = torch.full((M.shape[0], M.shape[1] + PAD), fill, dtype=torch.from_numpy(M).dtype, device=ctx.device)
    buf[:, :M.shape[1]] = torch.from_numpy(M).to(ctx.device)
    return buf[:, :M.shape[1]], buf


def output(ctx, I, dtype):
    """(view [5, I] for the five users, buffer [6, I + PAD]): the guard columns and a guard row hold SENTINEL."""
    buf = torch.full((U_STOP - U_START + 1, I + PAD), SENTINEL, dtype=dtype, device=ctx.device)
    return buf[:U_STOP - U_START, :I], buf


def check_output(buf, I, want):
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:, I:] == SENTINEL).all() and (got[-1] == SENTINEL).all()               # nothing stored outside [5, I]
    assert np.array_equal(bits(got[:-1, :I]), bits(want))


@pytest.mark.parametrize("I", SIZES)
def test_ease_scores(ctx, I):
    rs = np.random.RandomState(I)
    indptr, indices = rows_for(I, I + 1)
    vals = rs.normal(size=len(indices)).astype(np.float32)
    B = rs.normal(size=(I, I)).astype(np.float32)
    want = np.zeros((U_STOP - U_START, I), dtype=np.float32)
    for r, u in enumerate(range(U_START, U_STOP)):
        for e in range(indptr[u], indptr[u + 1]):
            want[r] = want[r] + vals[e] * B[indices[e]]                                 # float32 arrays: both roundings
    Bd, _ = padded(ctx, B, 3e38)                                                        # float32's POISON
    out, buf = output(ctx, I, torch.float32)
    ops.csr_dense_scores(ctx, ops.DeviceCSR(indptr, indices, I, ctx.device), ops.device_values(vals, ctx.device), Bd, U_START,
                         U_STOP, out=out)
    check_output(buf, I, want)


@pytest.mark.parametrize("I", SIZES)
def test_slope_scores(ctx, I):
    """A fifth of the table's cells are NaN (no common rater); for I > 1 target I // 2 has no other cell, so its score is the
    user's mean alone; user 4 has a NaN mean."""
    rs = np.random.RandomState(I)
    indptr, indices = rows_for(I, I + 2)
    T = rs.normal(size=(I, I))
    T[rs.rand(I, I) < 0.2] = np.nan
    if I > 1:
        T[:, I // 2] = np.nan
    mean = rs.uniform(1, 5, 7)
    mean[4] = np.nan
    want = np.zeros((U_STOP - U_START, I))
    for r, u in enumerate(range(U_START, U_STOP)):
        acc, cnt = np.zeros(I), np.zeros(I, dtype=np.int64)
        for e in range(indptr[u], indptr[u + 1]):
            row = T[indices[e]]
            keep = ~np.isnan(row)
            acc[keep] = acc[keep] + row[keep]
            cnt += keep
        with np.errstate(invalid="ignore", divide="ignore"):
            want[r] = np.where(cnt > 0, mean[u] + acc / cnt, mean[u])                   # one fp64 division, one addition
    assert I == 1 or (bits(want[3:, I // 2]) == bits(mean[5:7])).all()
    assert np.isnan(want[2]).all() and not np.isnan(want[3]).any()
    Td, _ = padded(ctx, T, POISON)
    out, buf = output(ctx, I, torch.float64)
    ops.slope_scores(ctx, ops.DeviceCSR(indptr, indices, I, ctx.device), torch.from_numpy(mean).to(ctx.device), Td, U_START, U_STOP,
                     out=out)
    check_output(buf, I, want)


@pytest.mark.parametrize("I", SIZES)
def test_bprslim_scores_skip_a_column_out_of_range(ctx, I):
    """Entry 10 of the long row names column I and entry 20 column -1: no row of St, skipped; the chain goes on behind them."""
    rs = np.random.RandomState(I)
    indptr, indices = rows_for(I, I + 3)
    indices[indptr[5] + 10], indices[indptr[5] + 20] = I, -1
    St = rs.normal(size=(I, I))
    want = np.zeros((U_STOP - U_START, I))
    for r, u in enumerate(range(U_START, U_STOP)):
        for e in range(indptr[u], indptr[u + 1]):
            if 0 <= indices[e] < I:
                want[r] = want[r] + St[indices[e]]
    _, Sbuf = padded(ctx, St, POISON)
    _, buf = output(ctx, I, torch.float64)
    ops.bprslim_scores(ctx, ops.DeviceCSR(indptr, indices, I, ctx.device), Sbuf, U_START, U_STOP, out=buf, I=I)
    check_output(buf, I, want)


@pytest.mark.parametrize("masked", [False, True], ids=["bprslim_table", "slope_table"])
@pytest.mark.parametrize("I", [1, 31, 32, 33, 65])
def test_transpose(ctx, I, masked):
    """dst[j, i] = src[i, j] (masked: a quiet NaN where freq[i, j] <= 0), every leading dimension wider than I."""
    rs = np.random.RandomState(I)
    src = rs.normal(size=(I, I))
    want = src.T.copy()
    dst = torch.full((I + 1, I + PAD), SENTINEL, dtype=torch.float64, device=ctx.device)
    sview, sbuf = padded(ctx, src, POISON)
    if masked:
        freq = rs.randint(-1, 3, size=(I, I)).astype(np.int32)
        bits(want)[freq.T <= 0] = QNAN
        ops.slope_table(ctx, padded(ctx, freq, 7)[0], sview, out=dst[:I, :I])
    else:
        ops.bprslim_table(ctx, sbuf, out=dst, I=I)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:, I:] == SENTINEL).all() and (got[I] == SENTINEL).all()
    assert np.array_equal(bits(got[:I, :I]), bits(want))
