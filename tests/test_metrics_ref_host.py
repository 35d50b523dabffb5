"""tests/helpers/metrics_ref.py pinned on the CPU: the per-user reference the device metric tests compare with agrees with the host
Evaluator, with the reference Evaluator's golden values and with rows worked out by hand; and the crafted lists of the
fragile-user tests keep their distance from the bound."""
import math

import numpy as np
import pytest

from tests.helpers import metrics_ref as mr


@pytest.mark.parametrize("cutoff,thr,frac_ratings", mr.RANDOM_CASES)
def test_ref_means_match_host_evaluator(cutoff, thr, frac_ratings):
    recs, ip, items, ratings = mr.random_case(cutoff, frac_ratings)
    got = mr.means(mr.rows(recs, ip, items, ratings, thr, cutoff))
    ref = mr.evaluator_means(recs, ip, items, ratings.astype(np.float64), thr, cutoff)
    for n in mr.NAMES:
        assert abs(got[n] - ref[n]) <= 1e-12, (n, got[n], ref[n])


def test_ref_means_match_golden(golden):
    g = golden("metrics_ref.npz")
    ip, k = g["test_indptr"], int(g["k"])
    ref = dict(zip(g["names"].tolist(), g["values"].tolist()))
    for cutoff in (k, 5):
        rws = mr.rows(g["recs"], ip, g["test_items"], g["test_ratings"], 0.0, cutoff)
        got = mr.means(rws)
        for n in mr.NAMES:
            assert abs(got[n] - ref[f"{n}@{cutoff}"]) <= 1e-12, (n, cutoff, got[n], ref[f"{n}@{cutoff}"])
        assert mr.sums(rws)[7] == g["recs"].shape[0]


def test_ref_rows_by_hand():
    """cutoff 4, implicit ratings, thr 1: every gain is 2^(1 - 1 + 1) - 1 = 1.
    user 0: one relevant item, recommended first; user 1: relevant {20, 21, 22}, 20 at rank 2 and 22 at rank 4;
    user 2: no test item."""
    ip = np.array([0, 1, 4, 4], np.int64)
    items = np.array([7, 20, 21, 22], np.int32)
    recs = np.array([[7, 1, 2, 3], [5, 20, -1, 22], [7, 20, 21, 22]], np.int32)
    d = [math.log(2) / math.log(r + 2) for r in range(4)]
    assert d[0] == 1.0
    dcg1, idcg1 = d[1] + d[3], 1.0 + d[1] + d[2]
    exp = np.array([
        [1.0, 0.25, 1.0, 1.0, (1 + 1 / 2 + 1 / 3 + 1 / 4) / 4, 1.0, 2 * 0.25 * 1.0 / 1.25, 1.0],
        [dcg1 / idcg1, 0.5, 2 / 3, 1.0, (0 + 1 / 2 + 1 / 3 + 2 / 4) / 4, 0.5, 2 * 0.5 * (2 / 3) / (0.5 + 2 / 3), 1.0],
        [0.0] * 8])
    got = mr.rows(recs, ip, items, None, 1.0, 4)
    assert np.allclose(got, exp, rtol=4e-16, atol=0), (got, exp)
    assert got[0, 6] == 0.4 and got[1, 5] == 0.5
    assert np.array_equal(got[2], np.zeros(8))
    # with thr above every rating nobody is valid; a user range inside the CSR reads its own rows
    assert not mr.rows(recs, ip, items, None, 1.5, 4).any()
    assert np.array_equal(mr.rows(recs[1:], ip, items, None, 1.0, 4, u_start=1), got[1:])
    s = mr.sums(got)
    assert s[7] == 2 and s[3] == 2 and s[1] == 0.75


def test_ref_gain_ranks_and_duplicates():
    """Explicit ratings: gain 2^(r - thr + 1) - 1; the IDCG takes the `cutoff` largest; a duplicate hits twice; a test item below
    the threshold neither hits nor counts."""
    ip = np.array([0, 4], np.int64)
    items = np.array([1, 2, 3, 4], np.int32)
    ratings = np.array([5.0, 2.0, 3.0, 4.0], np.float32)          # thr 3: item 2 is not relevant; gains 7, -, 1, 3
    recs = np.array([[3, 2, 3, 9]], np.int32)
    got = mr.rows(recs, ip, items, ratings, 3.0, 2)[0]            # cutoff 2 < ld: slots 3, 4 do not count
    d1 = math.log(2) / math.log(3)
    assert got[0] == 1.0 / (7.0 + 3.0 * d1) and got[1] == 0.5 and got[2] == 1 / 3 and got[5] == 1.0
    got = mr.rows(recs, ip, items, ratings, 3.0, 3)[0]
    assert got[1] == 2 / 3 and got[2] == 2 / 3 and got[4] == (1 + 1 / 2 + 2 / 3) / 3


@pytest.mark.parametrize("F", mr.FRAGILE_F)
@pytest.mark.parametrize("n", mr.FRAGILE_N)
def test_fragile_cases_keep_their_margin(F, n):
    """The device compares two fp64 values summed in another order than NumPy's: every crafted user must be further than
    FRAGILE_MARGIN (relative) from the bound, or the expected flag would depend on that order."""
    c = mr.fragile_case(F, n, mr.fragile_seed(F, n))
    assert c["margin"] > mr.FRAGILE_MARGIN, c["margin"]
    if n >= 5:
        assert c["counts"][1] == 3 and c["flags"][3] and not c["flags"][:3].any()
    if n > 100:
        assert 0.2 * n < c["counts"][0] < 0.8 * n              # both outcomes are well represented
