"""CPU: als_ref.backward_error and the cases of tests/helpers/als_cases.py, before any GPU holds el_als_solve to them.
  - on every edge case the restatement als_ref.half has a backward error of at most 2^-49 on every row: a condition on the inputs
    (a case beyond that is changed, not the bound), so that 16 times the restatement's own error is a bound worth having
  - no row's right-hand side is a cancelled sum (als_cases.Case says why that has to be a condition on the inputs)
  - the check has teeth: one entry dropped from one row's sums, or lambda added twice, raises that row's error above 1e-3
  - the long-row plan of each pattern has the rows and pieces its lengths say
  - the bad-pivot cases: the restatement refuses exactly rows 5 and 37, far from the edge of definiteness on both sides
"""
import numpy as np
import pytest

from tests.helpers import als_cases as ac
from tests.helpers import als_ref

PATTERNS = [("shared", F) for F in ac.SOLVE_F] + [(n, F) for F, NG in ((8, 16), (20, 4)) for n in ("1", str(NG - 1), str(NG), str(NG + 1))]
PATTERNS += [("no_short", 8)] + [(n, F) for n in ("long_ends", "all_long") for F in (8, 20, 65)]


@pytest.mark.parametrize("name,F", PATTERNS)
def test_restatement_backward_error_is_small_on_every_case(name, F):
    c = ac.case(name, F)
    print(name, F, "largest eta of the restatement %.3g" % c.eta_ref.max())
    assert c.eta_ref.max() <= 2.0 ** -49
    assert c.kappa.max() <= ac.KAPPA                                  # no row's b is a cancelled sum
    assert np.all(c.eta_ref[np.diff(c.indptr) == 0] == 0.0)          # an empty row: x = 0, b = 0
    assert ac.FLOOR <= c.bound <= 2.0 ** -45


def test_shared_case_is_the_stated_one():
    c = ac.case("shared", 16)
    assert np.diff(c.indptr).tolist() == [0, 1, 15, 16, 17, 32, 33, 47, 83, 0, 2, 7, 17, 16, 40, 1, 33, 64, 65, 3]
    assert c.Y.shape == (96, 16) and ac.PIECE == 16
    for r in range(c.U):
        row = c.indices[c.indptr[r]:c.indptr[r + 1]]
        assert np.all(np.diff(row) > 0) and (row.size == 0 or (0 <= row[0] and row[-1] < ac.I))
    assert ac.plan_counts(c.lens) == (10, 2 + 2 + 3 + 3 + 6 + 2 + 3 + 3 + 4 + 5)
    assert ac.plan_counts(ac.NO_SHORT_LENS)[0] == 14 and all(n > 16 or n == 0 for n in ac.NO_SHORT_LENS[16:32])
    assert all(n > 16 for n in ac.ALL_LONG_LENS) and ac.LONG_ENDS_LENS[0] > 16 and ac.LONG_ENDS_LENS[-1] > 16


def test_backward_error_by_hand():
    """F = 1, one row over two items: A = (4 + 9) + 2 * 4 + 0.5 = 21.5, b = 3 * 2 = 6."""
    Y = np.array([[2.0], [3.0]])
    indptr, indices = np.array([0, 1, 1], np.int64), np.array([0], np.int32)
    X = np.array([[6.0 / 21.5], [0.0]])
    eta = als_ref.backward_error(indptr, indices, Y, 2.0, 3.0, 0.5, X)
    assert eta[0] <= 2.0 ** -53 and eta[1] == 0.0
    X[0, 0] = 0.25                                       # |6 - 21.5 / 4| / (21.5 / 4 + 6)
    assert abs(als_ref.backward_error(indptr, indices, Y, 2.0, 3.0, 0.5, X, rows=[0])[0] - 0.625 / 11.375) <= 1e-16
    X[0, 0] = np.nan
    assert np.isnan(als_ref.backward_error(indptr, indices, Y, 2.0, 3.0, 0.5, X)[0])


@pytest.mark.parametrize("F", ac.SOLVE_F)
def test_a_dropped_entry_or_a_second_lambda_shows(F):
    c = ac.case("shared", F)
    G = c.Y.T.dot(c.Y)
    for r in (1, 4, 8, 19):                              # 1, 17, 83 and 3 entries
        idx = c.indices[c.indptr[r]:c.indptr[r + 1]]
        one = lambda ix, lam: als_ref.half(G, np.array([0, len(ix)], np.int64), ix, c.Y, ac.W_A, ac.W_B, lam, np.zeros((1, F)))[0]
        for what, x in (("dropped", one(idx[:-1], ac.LAM)), ("lambda twice", one(idx, 2 * ac.LAM))):
            X = c.X_ref.copy()
            X[r] = x
            eta = als_ref.backward_error(c.indptr, c.indices, c.Y, ac.W_A, ac.W_B, ac.LAM, X)
            print(F, r, what, "eta %.3g" % eta[r])
            assert eta[r] > 1e-3, (F, r, what, eta[r])
            others = np.arange(c.U) != r
            assert np.array_equal(eta[others], c.eta_ref[others])


@pytest.mark.parametrize("F", [8, 20])
@pytest.mark.parametrize("kind", ["indefinite", "nan"])
def test_bad_pivot_cases_are_far_from_the_edge(kind, F):
    c = ac.bad_case(kind, F)
    assert c.bad == sorted(ac.BAD_ROWS)
    has = [r for r in range(ac.BAD_U) if ac.BAD_ITEM in c.indices[c.indptr[r]:c.indptr[r + 1]]]
    assert has == sorted(ac.BAD_ROWS)
    G = c.Y.T.dot(c.Y)
    for r in range(ac.BAD_U):
        P = c.Y[c.indices[c.indptr[r]:c.indptr[r + 1]]]
        lo = np.linalg.eigvalsh(G + c.w_A * P.T.dot(P) + ac.LAM * np.eye(F))[0]
        if kind == "indefinite" and r in ac.BAD_ROWS:
            assert lo < -100.0, (r, lo)
        else:
            assert lo > 0.05, (r, lo)
    assert c.eta_ref[c.good].max() <= 2.0 ** -49
    assert ac.cancellation(c.indptr, c.indices, c.Y)[c.good].max() <= ac.KAPPA
