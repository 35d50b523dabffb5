"""GPU: el_profile_build (elliot_amd/csrc/el_attr.hip) and el_knn_build_f32 (el_knn.hip) against the reference's own matrices
(tests/golden/attr_ref.npz) and the restatement of their contract (tests/helpers/attr_ref.py), bit for bit.

Shapes: ATTR_TILE = 8192 fp64 cells per LDS tile, so 8192 + 37 features / targets cross one tile boundary; everything else is
as small as the path it reaches allows."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from elliot_amd.recommender import attribute_profiles as ap
from tests.helpers import attr_fixture as fxm
from tests.helpers import attr_ref

pytestmark = pytest.mark.gpu

TILE = 8192


@pytest.fixture(scope="module")
def fx(golden, tmp_path_factory):
    return fxm.load(golden("attr_ref.npz"), tmp_path_factory.mktemp("attr"))


# ---- el_profile_build ------------------------------------------------------------------------------------------------------------
PROFILES = {"auk_binary_A": ("binary", True), "auk_tfidf_A": ("tfidf", True), "vsm_binary_U": ("binary", False),
            "vsm_tfidf_U": ("tfidf", False)}


@pytest.mark.parametrize("tag", sorted(PROFILES))
def test_profiles_equal_the_reference_bit_for_bit(ctx, fx, tag):
    kind, by_len = PROFILES[tag]
    got = ap.user_profiles(ctx, fx.data, fx.data.side_information.ItemAttributes, kind, by_len)
    assert fxm.same_csr(got, fxm.csr(fx.z, tag))


@pytest.fixture(scope="module")
def edge_profiles():
    """nF = TILE + 37.  item 0: 200 features (more than one lane pass) on both sides of the tile boundary; item 1: four features
    that straddle it; items 2-4: no features; items 5-7: feature 100 with three different weights; the others 1-8 random features.
    user 0: only items without features; user 1: one item; user 2: 300 items; user 3: items 7, 5, 6 in that order -- the last
    writer of feature 100 is item 6; users 4..: 5-30 random items."""
    rs = np.random.RandomState(3)
    nF, I = TILE + 37, 400
    rows = [np.sort(rs.choice(np.arange(TILE - 220, TILE + 37), 200, replace=False)), np.array([TILE - 2, TILE - 1, TILE, TILE + 1]),
            np.zeros(0, int), np.zeros(0, int), np.zeros(0, int)]
    rows += [np.array([100, 7000 + j]) for j in range(3)]
    rows += [rs.choice(nF, rs.randint(1, 9), replace=False) for _ in range(I - len(rows))]
    rows = [r[rs.permutation(len(r))] for r in rows]                     # any order inside an item
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.concatenate(rows).astype(np.int32)
    F = sp.csr_matrix((np.ones(len(cols), np.float32), cols, indptr), shape=(I, nF))
    w = rs.uniform(0.05, 1.0, len(cols))
    users = [np.array([2, 3]), np.array([1]), rs.permutation(np.r_[0, 1, 8 + rs.permutation(I - 8)[:298]]), np.array([7, 5, 6])]
    users += [rs.permutation(I)[:rs.randint(5, 31)] for _ in range(20)]
    r_indptr = np.concatenate([[0], np.cumsum([len(u) for u in users])]).astype(np.int64)
    r_indices = np.concatenate(users).astype(np.int32)
    return r_indptr, r_indices, F, w


@pytest.mark.parametrize("mode,by_len", [("add", True), ("add", False), ("last", True), ("last", False)])
def test_profiles_at_the_edges_equal_the_restatement(ctx, edge_profiles, mode, by_len):
    r_indptr, r_indices, F, w = edge_profiles
    want = attr_ref.profile_matrix(r_indptr, r_indices, F, w, mode, by_len)
    got = ops.profile_build(ctx, r_indptr, r_indices, F, w if mode == "last" else None, mode, by_len)
    assert fxm.same_csr(got, want)
    assert got.indptr[1] == 0                                            # user 0: an empty row
    assert np.any(np.diff(got[2].indices) > 1) and got[2].indices.min() < TILE <= got[2].indices.max()
    if mode == "last":                                                   # user 3: feature 100 from item 6, its last writer
        e6 = F.indptr[6] + int(np.flatnonzero(F.indices[F.indptr[6]:F.indptr[7]] == 100)[0])
        assert got[3, 100] == np.float32(w[e6] / 3 if by_len else w[e6])
        summed = sum(w[F.indptr[i] + int(np.flatnonzero(F.indices[F.indptr[i]:F.indptr[i + 1]] == 100)[0])] for i in (5, 6, 7))
        assert got[3, 100] != np.float32(summed / 3 if by_len else summed)
    again = ops.profile_build(ctx, r_indptr, r_indices, F, w if mode == "last" else None, mode, by_len)
    assert fxm.same_csr(got, again)


def test_profile_build_refuses_bad_arguments(ctx):
    F = sp.csr_matrix(np.ones((3, 4), np.float32))
    ip, ix = np.array([0, 2], np.int64), np.array([0, 1], np.int32)
    with pytest.raises(ValueError, match="weight"):
        ops.profile_build(ctx, ip, ix, F, None, "last", True)
    with pytest.raises(ValueError, match="mode"):
        ops.profile_build(ctx, ip, ix, F, None, "sum", True)


# ---- el_knn_build_f32 --------------------------------------------------------------------------------------------------------
def w_host(W, vals):
    n = W.n_rows
    return sp.csr_matrix((vals[:W.nnz].cpu().numpy(), W.indices[:W.nnz].cpu().numpy(), W.indptr.cpu().numpy()), shape=(n, n))


@pytest.mark.parametrize("profile", ["binary", "tfidf"])
@pytest.mark.parametrize("sim", ["cosine", "dot"])
@pytest.mark.parametrize("N", [20, 300])
def test_w_of_the_golden_profiles_equals_the_restatement(ctx, fx, profile, sim, N):
    A = fxm.csr(fx.z, f"auk_{profile}_A")
    got = w_host(*ops.knn_build_f32(ctx, A, N, sim))
    assert fxm.same_csr(got, attr_ref.build_w(A, N, sim))
    assert fxm.same_csr(got, w_host(*ops.knn_build_f32(ctx, A, N, sim)))             # the same bytes on every run
    if N == 300:                                                                     # N >= n: nothing is cut, self-similarity kept
        assert np.all(got.diagonal() != 0)


def columns_equal(got, A, cols, N, sim):
    got = got.tocsc()
    for c, (x, v) in zip(cols, attr_ref.column_lists(A, cols, N, sim)):
        gx, gv = got.indices[got.indptr[c]:got.indptr[c + 1]], got.data[got.indptr[c]:got.indptr[c + 1]]
        order = np.argsort(x)
        assert np.array_equal(gx, x[order]) and np.array_equal(gv.view(np.uint32), v[order].view(np.uint32)), c


def test_w_across_a_tile_boundary(ctx):
    """TILE + 37 targets with 1-3 entries each: every column's neighbours come from both tiles, self on either side."""
    rs = np.random.RandomState(5)
    n, n_other = TILE + 37, 96
    rows = [np.sort(rs.choice(n_other, rs.randint(1, 4), replace=False)) for _ in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    A = sp.csr_matrix((rs.uniform(0.1, 1.0, indptr[-1]).astype(np.float32), np.concatenate(rows), indptr), shape=(n, n_other))
    cols = np.r_[0, 1, TILE - 1, TILE, TILE + 36, rs.choice(n, 40, replace=False)]
    for sim in ("cosine", "dot"):
        got = w_host(*ops.knn_build_f32(ctx, A, 10, sim))
        columns_equal(got, A, cols, 10, sim)


def test_w_of_long_rows_ties_zeros_and_empty_rows(ctx):
    """Feature 0 is carried by 5000 targets (a Q row of 5000 entries); target 0 has 600 entries (a P row of 600); targets 10 and
    11 are identical (an exact tie, cut by index); target 20 is empty; target 30 stores an explicit zero among its entries; target
    31 stores nothing but a zero."""
    rs = np.random.RandomState(9)
    n, n_other = 5200, 700
    rows, vals = [], []
    for c in range(n):
        k = 600 if c == 0 else rs.randint(1, 6)
        r = rs.choice(np.arange(1, n_other), k, replace=False)
        if c < 5000:
            r = np.r_[0, r]
        r = np.sort(r)
        rows.append(r)
        vals.append(rs.uniform(0.1, 1.0, len(r)).astype(np.float32))
    rows[11], vals[11] = rows[10].copy(), vals[10].copy()
    rows[20], vals[20] = np.zeros(0, int), np.zeros(0, np.float32)
    vals[30][len(vals[30]) // 2] = 0.0
    rows[31], vals[31] = np.array([0]), np.zeros(1, np.float32)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    A = sp.csr_matrix((np.concatenate(vals), np.concatenate(rows), indptr), shape=(n, n_other))
    assert A.nnz == indptr[-1]                                                        # the stored zeros are still stored
    cols = np.r_[0, 10, 11, 12, 20, 30, 31, 4999, 5000, 5199, rs.choice(n, 30, replace=False)]
    for sim in ("cosine", "dot"):
        got = w_host(*ops.knn_build_f32(ctx, A, 20, sim))
        columns_equal(got, A, cols, 20, sim)
        for empty in (20, 31):
            assert got[empty].nnz == 0 and got.tocsc()[:, empty].nnz == 0
        if sim == "cosine":                                                           # 10 and 11: cosine 1 with each other and with themselves
            gc = got.tocsc()
            assert {10, 11} <= set(gc.indices[gc.indptr[10]:gc.indptr[11]].tolist())


def test_binary_rows_give_the_integer_kernel_its_w(ctx, fx):
    A = fxm.csr(fx.z, "aik_A")
    f = w_host(*ops.knn_build_f32(ctx, A, 20, "dot"))
    i = w_host(*ops.knn_build(ctx, A, "user", 20, "dot"))
    assert fxm.same_csr(f, i)


def test_knn_build_f32_refuses_bad_arguments(ctx, dev):
    n, n_other = 3000, 4
    ip = torch.arange(n + 1, dtype=torch.int64, device=dev)
    ix = torch.zeros(n, dtype=torch.int32, device=dev)
    v = torch.ones(n, dtype=torch.float32, device=dev)
    qp = torch.tensor([0, n, n, n, n], dtype=torch.int64, device=dev)
    qi = torch.arange(n, dtype=torch.int32, device=dev)
    N = 8
    wp = torch.empty(n + 1, dtype=torch.int64, device=dev)
    wi = torch.empty(n * N, dtype=torch.int32, device=dev)
    wv = torch.empty(n * N, dtype=torch.float32, device=dev)
    need = int(ctx.lib.el_knn_f32_ws_bytes(n, N))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731

    def call(n_neighbors=N, p_indptr=p(ip), w_vals=p(wv), ws_ptr=p(ws), ws_bytes=need, sim=ops.KNN_SIMILARITIES["cosine"]):
        return ctx.lib.el_knn_build_f32(ctx.handle, ctx.stream(), p_indptr, p(ix), p(v), p(qp), p(qi), p(v), n, n_other, n_neighbors,
                                        sim, p(wp), p(wi), w_vals, ws_ptr, ws_bytes)
    assert call(n_neighbors=2049) != 0                                                # N > 2048
    assert call(p_indptr=None) != 0 and call(w_vals=None) != 0 and call(ws_ptr=None) != 0
    assert call(ws_bytes=need - 1) != 0
    assert call(sim=7) != 0
    assert call(n_neighbors=0) != 0
    assert call() == 0
    torch.cuda.synchronize()
    assert int(wp[-1].item()) == n * N                                                # all rows carry feature 0: N neighbours each
