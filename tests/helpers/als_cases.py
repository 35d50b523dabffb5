"""The small patterns that hold el_als_solve to its edges (tests/test_gpu_als_edges.py), their inputs, and what the NumPy restatement
(als_ref.half) gives on them.  tests/test_als_ref_host.py checks all of it without a GPU; the GPU test only reads it.

Every pattern is over I = 96 items with piece_len = 16, so a "long" row has 17 entries and a row of a few dozen has several pieces.
"""
import functools

import numpy as np

from tests.helpers import als_ref

I = 96
PIECE = 16
W_A, W_B, LAM = 1.5, 2.5, 0.1
FLOOR = 2.0 ** -52

# rows 0 and 9 empty; piece_len - 1, piece_len, piece_len + 1 (15, 16, 17); exact multiples of piece_len (32, 64); eight long rows;
# 20 rows: a last workgroup of 4 live rows at 16 rows per workgroup; at 4 rows per workgroup all five are full, and the dead lane
# groups of T = 64 are count_lens' (3 and 5 rows at F = 20)
SHARED_LENS = [0, 1, 15, 16, 17, 32, 33, 47, 83, 0, 2, 7, 17, 16, 40, 1, 33, 64, 65, 3]
SOLVE_F = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128]       # the ends of T = 16 (F <= 16), T = 64 (F <= 64), T = 256 (F <= 128)

# rows 16..31, one whole workgroup at F = 8, are long (17..48) or empty: its maxlen is 0
NO_SHORT_LENS = list(range(1, 17)) + [17, 19, 21, 0, 25, 27, 29, 31, 33, 35, 37, 0, 41, 43, 45, 48] + [5, 16, 1, 9, 2]
LONG_ENDS_LENS = [40, 3, 0, 5, 16, 33]                   # row 0 and the last row long
ALL_LONG_LENS = [17, 32, 33, 48, 95, 18, 20]


def count_lens(n):
    """n rows of 3..25 entries: short, long and, from 7 rows on, one of exactly piece_len."""
    return [(7 * i + 3) % 23 + 3 for i in range(n)]


def plan_counts(lens, piece_len=PIECE):
    """(n_long, n_pieces) of the long-row plan, from the lengths alone."""
    long_ = [n for n in lens if n > piece_len]
    return len(long_), sum(-(-n // piece_len) for n in long_)


def pattern(lens, seed=0, n_cols=I, without=()):
    """CSR of rows of the given lengths: each row's items drawn without replacement (never from `without`) and sorted."""
    rs = np.random.RandomState(seed)
    pool = np.setdiff1d(np.arange(n_cols), np.asarray(without, dtype=np.int64))
    rows = [np.sort(rs.choice(pool, n, replace=False)) for n in lens]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    return indptr, indices


def tables(n_rows, F, seed, n_cols=I):
    """Y ~ N(0, 0.1^2) [n_cols, F] and the X the solve starts from, N(0, 1) [n_rows, F]."""
    rs = np.random.RandomState(seed)
    return rs.normal(scale=0.1, size=(n_cols, F)), rs.normal(size=(n_rows, F))


def restated(indptr, indices, Y, w_A=W_A, rows=None):
    """als_ref.half, one row at a time, on the fp64 NumPy Gram: (X, eta, bad) -- the solution (zero rows where the Cholesky of the
    restatement refuses), its backward error per row (0 there) and the refused rows."""
    G = Y.T.dot(Y)
    U = len(indptr) - 1
    X = np.zeros((U, Y.shape[1]))
    bad = []
    for r in (range(U) if rows is None else rows):
        one = np.array([0, indptr[r + 1] - indptr[r]], np.int64)
        try:
            X[r] = als_ref.half(G, one, indices[indptr[r]:indptr[r + 1]], Y, w_A, W_B, LAM, np.zeros((1, Y.shape[1])))[0]
        except np.linalg.LinAlgError:
            bad.append(r)
    eta = als_ref.backward_error(indptr, indices, Y, w_A, W_B, LAM, X)
    eta[bad] = 0.0
    return X, eta, bad


def eta_bound(eta_half):
    """What a device row may reach: 16 times the restatement's largest backward error on the case (the margin for another, equally
    stable order of the sums and variant of Cholesky), and no less than one unit in the last place."""
    return max(16.0 * float(np.max(eta_half, initial=0.0)), FLOOR)


def cancellation(indptr, indices, Y):
    """Per row: max_c sum_j |y_jc| / max_c |sum_j y_jc|, the condition number of the sums behind |b|_inf (1 for an empty row)."""
    k = np.ones(len(indptr) - 1)
    for r in range(len(indptr) - 1):
        P = Y[indices[indptr[r]:indptr[r + 1]]]
        if P.shape[0]:
            k[r] = np.abs(P).sum(axis=0).max() / np.abs(P.sum(axis=0)).max()
    return k


KAPPA = 32.0


class Case:
    """A pattern of rows of the given lengths, its tables and the restatement on them.  The backward error weighs the residual
    against |b|_inf, and b is a sum of signed terms: where it nearly cancels (a few dozen N(0, s^2) terms at F = 1 do now and then)
    the error of ANY order of that sum is its condition number times a few ulps, in the restatement as on the device, and the
    two stop being comparable by a fixed factor.  So the tables are redrawn until every row's sum has a condition number of at
    most KAPPA: a condition on the inputs alone."""

    def __init__(self, lens, F, seed=0):
        self.lens, self.F = list(lens), F
        self.indptr, self.indices = pattern(lens, seed)
        self.U = len(lens)
        for draw in range(100):
            self.Y, self.X0 = tables(self.U, F, 1000 * (draw + 1) + F + seed)
            self.kappa = cancellation(self.indptr, self.indices, self.Y)
            if self.kappa.max() <= KAPPA:
                break
        self.X_ref, self.eta_ref, bad = restated(self.indptr, self.indices, self.Y)
        assert not bad
        self.bound = eta_bound(self.eta_ref)


@functools.lru_cache(maxsize=None)
def case(name, F):
    """The named pattern at F factors, restated once and shared (nobody writes to it)."""
    lens = {"shared": SHARED_LENS, "no_short": NO_SHORT_LENS, "long_ends": LONG_ENDS_LENS, "all_long": ALL_LONG_LENS}.get(name)
    if lens is None:
        lens = count_lens(int(name))                      # "1", "15", ...: a row count
    return Case(lens, F)


# ---- bad pivots -----------------------------------------------------------------------------------------------------------------
BAD_ITEM = 11
BAD_ROWS = (5, 37)
BAD_U = 48
BAD_I = 400              # enough items that G - 3 S_r stays well inside the positive definite cone on a row of a few entries


class BadCase:
    """48 short rows over BAD_I items; BAD_ITEM is in rows 5 and 37 and nowhere else.
      kind "indefinite": w_A = -3 and Y[BAD_ITEM] scaled to 100 times the norm of the rest of Y, so A_r = G - 3 S_r is far from
                         positive definite exactly where the item is
      kind "nan":        w_A = 1.5, a clean Y (and Gram); the solve is handed Y with one NaN in row BAD_ITEM"""

    def __init__(self, kind, F):
        self.kind, self.F = kind, F
        lens = [i % 3 + 1 for i in range(BAD_U)]
        indptr, indices = pattern(lens, 3, n_cols=BAD_I, without=(BAD_ITEM,))
        rows = [indices[indptr[r]:indptr[r + 1]] for r in range(BAD_U)]
        for r in BAD_ROWS:
            rows[r] = np.sort(np.append(rows[r], BAD_ITEM)).astype(np.int32)
        self.indptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
        self.indices = np.concatenate(rows).astype(np.int32)
        self.Y, self.X0 = tables(BAD_U, F, 77 + F, n_cols=BAD_I)
        self.w_A = W_A
        if kind == "indefinite":
            self.w_A = -3.0
            rest = np.delete(self.Y, BAD_ITEM, axis=0)
            self.Y[BAD_ITEM] *= 100.0 * np.linalg.norm(rest) / np.linalg.norm(self.Y[BAD_ITEM])
        self.good = [r for r in range(BAD_U) if r not in BAD_ROWS]
        self.Y_solve = self.Y
        if kind == "nan":
            self.Y_solve = self.Y.copy()
            self.Y_solve[BAD_ITEM, F // 2] = np.nan
        # the restatement on what the solve is handed decides which rows are refused (a NaN pivot passes np.linalg.cholesky's own
        # test on some LAPACKs, so there the rows that hold the NaN are the refused ones)
        self.X_ref, self.eta_ref, self.bad = restated(self.indptr, self.indices, self.Y, self.w_A)
        if kind == "nan":
            assert not self.bad
            self.bad = [r for r in range(BAD_U) if BAD_ITEM in self.indices[self.indptr[r]:self.indptr[r + 1]]]
            self.eta_ref[self.bad] = 0.0
        self.bound = eta_bound(self.eta_ref[self.good])


@functools.lru_cache(maxsize=None)
def bad_case(kind, F):
    return BadCase(kind, F)
