"""GPU: el_lu_f64 / el_inv_f64 (elliot_amd/csrc/el_ease.hip) at the edges of their kernels, with the matrices and the condition-scaled
bound of tests/test_gpu_ease.py (matrix, check_inverse).
  panels and tiles   INV_NB = INV_TILE = 64: n = 2, 63, 64, 65 (a last panel of 63 columns, of one; a trailing update of one row and
                     column), 127, 128, 129, 193; general, and zero_diag where every step swaps; the factorisation alone picks the
                     same pivots and its packed L and U give back the permuted A
  lda > n            both entry points on a [n, n + 3] buffer: the same bits as the contiguous run, the padding untouched
  ties               k_lu_pivot keeps the smallest row among equal |a|: within one thread's rows (j + tid and j + tid + 1024),
                     across the lanes of a wave, across the 16 waves
  NaN                reported for its own column, before the panel's end and two panels on
"""
import ctypes as C

import numpy as np
import pytest
import torch

from elliot_amd import ops
from tests.test_gpu_ease import check_inverse, dev, matrix

pytestmark = pytest.mark.gpu

EDGE_N = [2, 63, 64, 65, 127, 128, 129, 193]


def row_order(ipiv):
    """The rows of A in the order getrf's successive swaps leave them."""
    perm = np.arange(ipiv.shape[0])
    for j, p in enumerate(ipiv):
        perm[j], perm[p] = perm[p], perm[j]
    return perm


@pytest.mark.parametrize("kind", ["general", "zero_diag"])
@pytest.mark.parametrize("n", EDGE_N)
def test_panel_and_tile_edges(ctx, kind, n):
    A = matrix(kind, n, 3 * n + 1)
    ipiv, X = check_inverse(ctx, A)
    if kind == "zero_diag":
        assert ipiv[0] != 0
    assert np.all(ipiv >= np.arange(n)) and np.all(ipiv < n)
    Ad = dev(A, ctx, np.float64)
    ipiv_lu = ops.lu_f64(ctx, Ad).cpu().numpy()
    assert np.array_equal(ipiv_lu, ipiv)
    LU = Ad.cpu().numpy()
    L, U = np.tril(LU, -1) + np.eye(n), np.triu(LU)
    PA = A[row_order(ipiv)]
    assert np.abs(L).max() <= 1.0                         # partial pivoting
    cond = np.abs(A).sum(axis=0).max() * np.abs(np.linalg.inv(A)).sum(axis=0).max()
    assert np.abs(L @ U - PA).max() <= max(cond, 1.0) * 1e-14 * np.abs(A).max()
    # and element by element what any order of the sums of an LU guarantees: |L U - P A| <= gamma_n |L| |U| (Higham, Theorem 9.3)
    gamma = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
    Ll, Ul = L.astype(np.longdouble), U.astype(np.longdouble)            # (so that the host's own products do not count)
    slack = np.abs(Ll @ Ul - PA) - gamma * (np.abs(Ll) @ np.abs(Ul))
    assert slack.max() <= 0.0, np.unravel_index(slack.argmax(), slack.shape)


@pytest.mark.parametrize("n", [65, 129])
def test_padded_layout(ctx, n):
    """lda = n + 3 through the C ABI, as ops.inv_f64 / ops.lu_f64 call it: pivot swap, TRSM, MFMA update and the final copy all
    honour it."""
    A = matrix("zero_diag", n, 5 * n)
    lda, sentinel = n + 3, -12345.678
    p = lambda t: C.c_void_p(t.data_ptr())
    for what in ("inv", "lu"):
        flat = dev(A, ctx, np.float64)
        ipiv_flat = (ops.inv_f64 if what == "inv" else ops.lu_f64)(ctx, flat).cpu().numpy()
        host = np.full((n, lda), sentinel)
        host[:, :n] = A
        buf = dev(host, ctx, np.float64)
        ipiv = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
        status = torch.empty(1, dtype=torch.int32, device=ctx.device)
        if what == "inv":
            need = int(ctx.lib.el_inv_f64_ws_bytes(n))
            ws = torch.empty(need, dtype=torch.uint8, device=ctx.device)
            rc = ctx.lib.el_inv_f64(ctx.handle, ctx.stream(), p(buf), lda, n, p(ipiv), p(status), p(ws), need)
        else:
            rc = ctx.lib.el_lu_f64(ctx.handle, ctx.stream(), p(buf), lda, n, p(ipiv), p(status))
        ops._lib.check(rc, what)
        assert int(status.item()) == 0x7fffffff
        got = buf.cpu().numpy()
        assert got[:, :n].tobytes() == flat.cpu().numpy().tobytes(), what
        assert np.array_equal(ipiv.cpu().numpy(), ipiv_flat), what
        assert np.all(got[:, n:] == sentinel), what


@pytest.mark.parametrize("rows,want", [((1030, 70, 6, 64), 6), ((1030, 70), 70), ((1030, 1029), 1029)])
def test_pivot_ties_go_to_the_smallest_row(ctx, rows, want):
    """Column 0 of a 1100 x 1100 matrix holds +-7.0 in the planted rows and less than 1 elsewhere.  At j = 0 thread t scans rows t and
    t + 1024: rows 6 and 1030 are one thread's, 70 and 64 another wave's, 1029 a neighbouring lane's."""
    n = 1100
    A = matrix("general", n, 11)
    A[:, 0] *= 0.9 / np.abs(A[:, 0]).max()
    for i, r in enumerate(rows):
        A[r, 0] = 7.0 if i % 2 == 0 else -7.0
    assert np.sum(np.abs(A[:, 0]) == 7.0) == len(rows) and np.sort(np.abs(A[:, 0]))[-len(rows) - 1] < 1.0
    ipiv, _ = check_inverse(ctx, A)
    assert ipiv[0] == want == min(rows)
    Ad = dev(A, ctx, np.float64)
    assert np.array_equal(ops.lu_f64(ctx, Ad).cpu().numpy(), ipiv)


@pytest.mark.parametrize("col", [3, 100])
def test_nan_is_reported_for_its_column(ctx, col):
    """One NaN at (5, col) of a 130 x 130 matrix.  Until column `col` is reached no earlier column holds a NaN: it stays in its own
    column of its row, or, once that row is a pivot row, fills the column below it -- either way the pivot of `col` is NaN."""
    A = matrix("general", 130, 17)
    A[5, col] = np.nan
    for f in (ops.inv_f64, ops.lu_f64):
        with pytest.raises(np.linalg.LinAlgError, match=r"column %d\b" % col):
            f(ctx, dev(A, ctx, np.float64))
    check_inverse(ctx, matrix("general", 130, 17))
