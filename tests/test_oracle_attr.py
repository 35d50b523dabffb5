"""The restatement of the attribute kernels (tests/helpers/attr_ref.py) pinned to the reference's own output
(tests/golden/attr_ref.npz, scripts/gen_golden_attr.py): W per column, scores and top-k given the reference's W, VSM's score matrix.

The user-profile cases compare a float32 chain (the reference: sklearn normalises both float32 rows, scipy multiplies in float32)
with fp64 sums rounded once (ours), so values agree within attr_ref.bound(L) = (2 L + 8) 2^-24 relative, L = the longest
profile row; measured by the generator: 3.0e-7 at L = 37 (`<case>_err`).  AttributeItemKNN's matrix is binary: its W is compared
as tests/test_oracle_knn.py compares ItemKNN's."""
import numpy as np
import pytest

from tests.helpers import attr_fixture as fxm
from tests.helpers import attr_ref, knn_ref

AUK = [(p, s) for p in ("binary", "tfidf") for s in ("cosine", "dot")]
VSM = [(u, i) for u in ("binary", "tfidf") for i in ("binary", "tfidf")]


@pytest.fixture(scope="module")
def fx(golden, tmp_path_factory):
    return fxm.load(golden("attr_ref.npz"), tmp_path_factory.mktemp("attr"))


@pytest.mark.parametrize("profile,sim", AUK)
def test_user_profile_w_matches_reference(fx, profile, sim):
    z, tag = fx.z, f"auk_{profile}_{sim}"
    A = fxm.csr(z, f"auk_{profile}_A")
    N, L = int(z["n_neighbors"]), int(np.diff(A.indptr).max())
    assert L == int(z[f"{tag}_L"])
    rtol = attr_ref.bound(L)
    assert float(z[f"{tag}_err"]) <= rtol                                  # what the generator measured sits inside the bound
    ours = attr_ref.column_lists(A, np.arange(A.shape[0]), N, sim)
    strict, total = attr_ref.compare_columns(fxm.w_lists(z, tag), ours, rtol, N)
    print(f"{tag}: L {L} bound {rtol:.3e} measured {float(z[f'{tag}_err']):.3e} index-compared {strict}/{total}")
    assert strict >= 0.9 * total                                           # the near-cut band leaves out at most 10 % of the entries
    assert sum(len(x) == N for x, _ in ours) > A.shape[0] // 2, "the neighbour cut must bind on most columns"


@pytest.mark.parametrize("sim", ["cosine", "dot"])
def test_item_attribute_w_matches_reference(fx, sim):
    """As test_oracle_knn.test_w_columns_match_reference: the binary item x feature matrix through the integer contract."""
    z, tag = fx.z, f"aik_{sim}"
    A = fxm.csr(z, "aik_A")
    N = int(z["n_neighbors"])
    M = knn_ref.targets_matrix(A, "user")                                  # rows of A = the targets
    lists = knn_ref.column_lists(M, np.arange(M.shape[0]), N, sim)
    rtol = 1e-5 if sim == "cosine" else 0.0
    binding = 0
    for c, ((rx, rv), (ox, ov)) in enumerate(zip(fxm.w_lists(z, tag), lists)):
        assert len(rx) == len(ox), c
        if not len(rx):
            continue
        binding += len(ox) == N
        order = np.lexsort((rx, -rv.astype(np.float64)))
        rx, rv = rx[order], rv[order]
        if sim == "dot":
            assert np.array_equal(ov, rv), c
        else:
            np.testing.assert_allclose(ov, rv, rtol=rtol, atol=0)
        cut = rv.min()
        near_o, near_r = np.abs(ov - cut) <= rtol * abs(cut), np.abs(rv - cut) <= rtol * abs(cut)
        assert set(ox[~near_o].tolist()) == set(rx[~near_r].tolist()), c
    assert binding > M.shape[0] // 2, "the neighbour cut must bind on most columns"


@pytest.mark.parametrize("tag,side", [(f"aik_{s}", "item") for s in ("cosine", "dot")] + [(f"auk_{p}_{s}", "user") for p, s in AUK])
def test_scores_and_lists_match_reference_given_its_w(fx, tag, side):
    z, R = fx.z, fx.data.sp_i_train_ratings
    preds = knn_ref.scores(R, fxm.w_csr(z, tag), side)
    idx, val = knn_ref.topk(preds, np.arange(R.shape[0]), int(z["k"]), excl=(R.indptr, R.indices))
    ri, rv = z[f"{tag}_rec_idx"], z[f"{tag}_rec_val"]
    assert np.array_equal(val.view(np.uint32), rv.view(np.uint32))
    assert knn_ref.cut_ties_equal(idx, val, ri, rv)


@pytest.mark.parametrize("up,ip", VSM)
def test_vsm_scores_and_lists_match_reference(fx, up, ip):
    z, tag = fx.z, f"vsm_{up}_{ip}"
    ours, ref = attr_ref.vsm_scores(fxm.csr(z, f"vsm_{up}_U"), fxm.csr(z, f"vsm_{ip}_I")).astype(np.float64), z[f"{tag}_sim"].astype(np.float64)
    L = int(max(np.diff(z[f"vsm_{up}_U_indptr"]).max(), np.diff(z[f"vsm_{ip}_I_indptr"]).max()))
    rtol = attr_ref.bound(L)
    assert np.array_equal(ours == 0, ref == 0)
    worst = float(np.max(np.abs(ours - ref)[ref != 0] / np.abs(ref[ref != 0])))
    print(f"{tag}: L {L} bound {rtol:.3e} measured {worst:.3e}")
    assert worst <= rtol
    R = fx.data.sp_i_train
    k = int(z["k"])
    idx, val = knn_ref.topk(ours.astype(np.float32), np.arange(R.shape[0]), k, excl=(R.indptr, R.indices))
    ri, rv = z[f"{tag}_rec_idx"], z[f"{tag}_rec_val"]
    assert np.array_equal(idx >= 0, ri >= 0)
    for u in range(R.shape[0]):
        n = int((idx[u] >= 0).sum())
        o, r = val[u, :n].astype(np.float64), rv[u, :n].astype(np.float64)
        assert np.all(np.abs(o - r) <= rtol * np.abs(r)), u
        last = min(o[-1], r[-1]) if n else 0.0                             # near-ties with the list's last value may swap places
        far_o, far_r = o > last + 2 * rtol * abs(last), r > last + 2 * rtol * abs(last)
        # inside the list, entries closer than the bound may swap places too: compare the sets of every value band
        assert set(idx[u, :n][far_o].tolist()) <= set(ri[u, :n].tolist()) and set(ri[u, :n][far_r].tolist()) <= set(idx[u, :n].tolist()), u
