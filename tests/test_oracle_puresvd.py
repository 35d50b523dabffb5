"""CPU: the NumPy fp64 restatement of the device's PureSVD (tests/helpers/psvd_ref.py) against the reference's own runs recorded in
tests/golden/puresvd_ref.npz (scripts/gen_golden_puresvd.py).

The yardstick of every case is D = max |P_ref32 - P_ref64|, P = user_vec item_vec^T: what the reference computes on its float32
matrix against the same code on the float64 copy.  An fp64 pipeline started from the reference's own float32-rounded start matrix
must not be further from the float64 answer than the reference's float32 arithmetic is, so the bound on the scores is 1 x D --
derived, not tuned (measured here: 0.001 to 0.027 x D, of which up to 0.013 x D is the float32 rounding of the stored table).
P_ref64 is rebuilt from the stored table (psvd_ref.ref64_tables); the error of that rebuilding, recorded in the file, is added to
the measured distance before it is compared with D."""
import numpy as np
import pytest

from tests.helpers import psvd_ref

CASES = ["u300_i200_f10_s42", "u200_i320_f10_s42", "u400_i250_f32_s42", "u150_i120_f16_s42", "u1000_i600_f50_s42",
         "u600_i900_f100_s42", "u150_i120_f16_s7"]
K = 10


@pytest.fixture(scope="module")
def g(golden):
    return golden("puresvd_ref.npz")


@pytest.fixture(scope="module")
def restated(g):
    cache = {}

    def get(tag):
        if tag not in cache:
            A = psvd_ref.csr_of(g, tag)
            cache[tag] = (A, psvd_ref.restate(A, int(g[f"{tag}_factors"]), int(g[f"{tag}_seed"])))
        return cache[tag]
    return get


def test_golden_lists_every_case(g):
    assert list(g["cases"]) == CASES


@pytest.mark.parametrize("tag", CASES)
def test_scores_within_the_references_own_error(g, restated, tag):
    A, r = restated(tag)
    D, rebuild = float(g[f"{tag}_D"]), float(g[f"{tag}_rebuild_err"])
    P64 = psvd_ref.scores(*psvd_ref.ref64_tables(g, tag, A))
    for name, user, item in (("fp64 tables", r["user64"], r["item64"]), ("float32 tables", r["user32"], r["item32"])):
        err = float(np.abs(psvd_ref.scores(user, item) - P64).max()) + rebuild
        print(f"{tag}: {name}: max |P - P_ref64| = {err / D:.4g} D (D = {D:.3g}, of which rebuilding {rebuild / D:.3g} D)")
        assert err <= D, (tag, name, err, D)


@pytest.mark.parametrize("tag", CASES)
def test_singular_values(g, restated, tag):
    _, r = restated(tag)
    s32, s64 = g[f"{tag}_sigma32"], g[f"{tag}_sigma64"]
    mine, ref = float(np.abs(r["sigma"] - s64).max()), float(np.abs(s32 - s64).max())
    print(f"{tag}: max |sigma - sigma_ref64| = {mine:.3g} (relative {mine / s64.max():.3g}); the reference's float32 run: {ref:.3g}")
    assert mine <= ref


@pytest.mark.parametrize("tag", CASES)
def test_signs_equal_the_references(g, restated, tag):
    A, r = restated(tag)
    user64, _ = psvd_ref.ref64_tables(g, tag, A)
    dots = np.einsum("uc,uc->c", r["user64"], user64)          # both tables have unit columns
    strong = np.abs(dots) > 0.9
    print(f"{tag}: components with |<u, u_ref>| > 0.9: {int(strong.sum())} of {dots.size}, smallest |dot| {np.abs(dots).min():.6f}")
    assert strong.sum() >= 0.9 * dots.size
    assert (dots[strong] > 0).all(), np.flatnonzero(strong & (dots <= 0))


@pytest.mark.parametrize("tag", CASES)
def test_lists_equal_the_float64_references(g, restated, tag):
    A, r = restated(tag)
    P64 = psvd_ref.scores(*psvd_ref.ref64_tables(g, tag, A))
    weak = psvd_ref.fragile(P64, g[f"{tag}_row_err"], A.indptr, A.indices, K)
    print(f"{tag}: fragile users {int(weak.sum())} of {A.shape[0]}")
    assert weak.sum() <= 0.02 * A.shape[0]
    mine, _ = psvd_ref.topk(psvd_ref.scores(r["user64"], r["item64"]), A.indptr, A.indices, K)
    ref = g[f"{tag}_top64"].astype(np.int32)
    bad = [u for u in np.flatnonzero(~weak) if not np.array_equal(mine[u], ref[u])]
    assert not bad, (tag, bad[:10])


@pytest.mark.parametrize("tag", CASES)
def test_generator_assertions_hold_in_the_file(g, tag):
    A = psvd_ref.csr_of(g, tag)
    U, I = A.shape
    f = int(g[f"{tag}_factors"])
    assert np.diff(A.indptr).min() > 0 and np.diff(A.tocsc().indptr).min() > 0
    assert np.linalg.matrix_rank(A.toarray().astype(np.float64)) >= f + 10
    assert g[f"{tag}_top32_rows"].shape[0] <= 0.02 * U
    assert g[f"{tag}_sigma32"].shape == g[f"{tag}_sigma64"].shape == (f,)
    assert g[f"{tag}_t64"].shape == (max(U, I), f) and g[f"{tag}_top64"].shape == (U, K)
    assert 0 < float(g[f"{tag}_D"]) < 1e-3 and float(g[f"{tag}_rebuild_err"]) <= 0.05 * float(g[f"{tag}_D"])


def test_cases_cover_both_orientations_and_both_iteration_counts(g):
    plans = {tag: psvd_ref.plan(*(int(x) for x in g[f"{tag}_shape"]), int(g[f"{tag}_factors"])) for tag in CASES}
    assert {p[1] for p in plans.values()} == {4, 7} and {p[2] for p in plans.values()} == {False, True}


def test_the_seed_reaches_the_start_matrix(g, restated):
    a, b = "u150_i120_f16_s42", "u150_i120_f16_s7"
    assert np.array_equal(g[f"{a}_indices"], g[f"{b}_indices"]) and int(g[f"{a}_seed"]) != int(g[f"{b}_seed"])
    assert not np.array_equal(restated(a)[1]["user64"], restated(b)[1]["user64"])
    assert not np.array_equal(g[f"{a}_sigma64"], g[f"{b}_sigma64"])
