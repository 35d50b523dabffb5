"""el_knn_build / el_knn_score_topk (csrc/el_knn.hip) against the restatement (tests/helpers/knn_ref.py) and the reference's
own W and lists (tests/golden/knn_{item,user}_ref.npz)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.helpers import knn_ref

pytestmark = pytest.mark.gpu

CASES = [(side, sim, b) for side in ("item", "user") for sim in ("cosine", "dot") for b in (False, True)]


def fixture_matrix(golden, side, binary):
    z = golden(f"knn_{side}_ref.npz")
    R = sp.csr_matrix((z["R_data"], z["R_indices"], z["R_indptr"]), shape=tuple(z["shape"]))
    if binary:
        R = R.copy()
        R.data[:] = 1.0
    return z, R


def host_w(W, vals):
    n = W.n_rows
    return sp.csr_matrix((vals[:W.nnz].cpu().numpy(), W.indices[:W.nnz].cpu().numpy(), W.indptr.cpu().numpy()), shape=(n, n))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_w_equal(Wd, Wr):
    assert np.array_equal(Wd.indptr, Wr.indptr)
    assert np.array_equal(Wd.indices, Wr.indices)
    assert same_bits(Wd.data, Wr.data)


def operands(ops, ctx, R, W, side):
    Rd, Rv = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], ctx.device), ops.device_values(R.data, ctx.device)
    W = W.tocsr()
    W.sort_indices()
    Wd, Wv = ops.DeviceCSR(W.indptr, W.indices, W.shape[1], ctx.device), ops.device_values(W.data, ctx.device)
    return (Rd, Rv, Wd, Wv) if side == "item" else (Wd, Wv, Rd, Rv)


@pytest.mark.parametrize("side,sim,binary", CASES)
@pytest.mark.parametrize("N", [20, 1000])
def test_build_matches_restatement(ctx, golden, side, sim, binary, N):
    from elliot_amd import ops
    _, R = fixture_matrix(golden, side, binary)
    W, vals = ops.knn_build(ctx, R, side, N, sim)
    torch.cuda.synchronize()
    assert_w_equal(host_w(W, vals), knn_ref.build_w(R, side, N, sim))


@pytest.mark.parametrize("side,sim,binary", CASES)
def test_scoring_on_reference_w_matches_reference_lists(ctx, golden, side, sim, binary):
    from elliot_amd import ops
    z, R = fixture_matrix(golden, side, binary)
    tag = f"{sim}_{'bin' if binary else 'rat'}"
    n = z[f"{tag}_w_indptr"].shape[0] - 1
    Wref = sp.csc_matrix((z[f"{tag}_w_data"], z[f"{tag}_w_indices"], z[f"{tag}_w_indptr"]), shape=(n, n), dtype=np.float32)
    A, Av, B, Bv = operands(ops, ctx, R, Wref, side)
    excl = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], ctx.device)
    k = int(z["k"])
    idx, val = ops.knn_score_topk(ctx, A, Av, B, Bv, 0, R.shape[0], k, excl=excl)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    ri, rv = z[f"{tag}_rec_idx"], z[f"{tag}_rec_val"]
    assert same_bits(val, rv)
    assert knn_ref.cut_ties_equal(idx, val, ri, rv)


def random_cand(R, per_user, seed):
    rs = np.random.RandomState(seed)
    U, I = R.shape
    rows = [np.sort(rs.choice(I, size=per_user, replace=False)).astype(np.int32) for _ in range(U)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows)


@pytest.mark.parametrize("side,sim,binary", CASES)
def test_scoring_on_device_w_matches_restatement(ctx, golden, side, sim, binary):
    from elliot_amd import ops
    _, R = fixture_matrix(golden, side, binary)
    W, Wv = ops.knn_build(ctx, R, side, 20, sim)
    Wh = host_w(W, Wv)
    users = np.arange(R.shape[0])
    preds = knn_ref.scores(R, Wh, side)
    Rd, Rv = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], ctx.device), ops.device_values(R.data, ctx.device)
    A, Av, B, Bv = (Rd, Rv, W, Wv) if side == "item" else (W, Wv, Rd, Rv)
    excl = (R.indptr, R.indices)
    cand = random_cand(R, 6, seed=3)
    for kind, k in (("excl", 10), ("excl", 140), ("cand", 4), ("cand", 10)):       # k = 10 > 6 candidates: padding
        m = excl if kind == "excl" else cand
        dm = ops.DeviceCSR(m[0], m[1], R.shape[1], ctx.device)
        # two blocks, as RecMixin asks for them
        got = [ops.knn_score_topk(ctx, A, Av, B, Bv, s, e, k, **{kind: dm}) for s, e in ((0, 77), (77, R.shape[0]))]
        idx = np.concatenate([g[0].cpu().numpy() for g in got])
        val = np.concatenate([g[1].cpu().numpy() for g in got])
        ei, ev = knn_ref.topk(preds, users, k, **{kind: m})
        assert np.array_equal(idx, ei), (kind, k)
        assert same_bits(val, ev), (kind, k)
    assert (idx[:, 6:] == -1).all() and np.isneginf(val[:, 6:]).all()


SELECT_I = 1000


@pytest.fixture(scope="module")
def select_case():
    """Three users with one entry of A each, onto three dense rows of B: strictly ascending in the item index (every element beats
    the threshold, the buffer compacts in every pass), strictly descending (nothing enters after the first compaction), long runs
    of equal values (the index decides).  Returns (A, B, preds = scipy's A.dot(B))."""
    item = np.arange(SELECT_I)
    rows = np.stack([(item + 1) / 8.0, (SELECT_I - item) / 8.0, ((item // 97) * 7 % 5 + 1) / 4.0]).astype(np.float32)
    A = sp.csr_matrix((np.array([1.0, 2.0, 0.5], np.float32), np.arange(3), np.arange(4)), shape=(3, 3))
    B = sp.csr_matrix(rows)
    assert B.nnz == 3 * SELECT_I
    return A, B, np.asarray(A.dot(B).toarray(), np.float32)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 448])
def test_running_selection_at_its_capacity_steps(ctx, select_case, k):
    """The one-wave stream-select of k_knn_score at k = 1, around the step of its capacity from 128 to 256 slots (63, 64, 65) and at
    448 (512 slots exactly), on the three orders of `select_case`; once with an exclusion row, once with k - 1 candidates, so that
    every list ends in (-1, -inf).  (k = 10 and 140 on rating data: test_scoring_on_device_w_matches_restatement.)"""
    from elliot_amd import ops
    A, B, preds = select_case
    Ad, Av = ops.DeviceCSR(A.indptr, A.indices, 3, ctx.device), ops.device_values(A.data, ctx.device)
    Bd, Bv = ops.DeviceCSR(B.indptr, B.indices, SELECT_I, ctx.device), ops.device_values(B.data, ctx.device)
    rs = np.random.RandomState(k)
    users = np.arange(3)
    for kind, per_user in (("excl", 37), ("cand", k - 1)):
        rows = [np.sort(rs.choice(SELECT_I, size=per_user, replace=False)).astype(np.int32) for _ in users]
        if kind == "excl":
            rows = [np.union1d(r, [0, SELECT_I - 1]).astype(np.int32) for r in rows]         # the best item of two of the rows
        m = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32))
        dm = ops.DeviceCSR(m[0], m[1], SELECT_I, ctx.device)
        idx, val = ops.knn_score_topk(ctx, Ad, Av, Bd, Bv, 0, 3, k, **{kind: dm})
        ei, ev = knn_ref.topk(preds, users, k, **{kind: m})
        assert np.array_equal(idx.cpu().numpy(), ei), kind
        assert same_bits(val.cpu().numpy(), ev), kind
        if kind == "cand":
            assert (ei[:, k - 1] == -1).all() and np.isneginf(ev[:, k - 1]).all()


def test_large_catalogue_tiles_build_and_scoring(ctx):
    """120 K items: more than one LDS tile in both kernels (64 KiB of accumulators = 16 K items).  64 sampled columns of W and
    256 sampled users' lists bit-exact against the restatement."""
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    U, I, N, k = 30000, 120000, 20, 10
    indptr, indices = zipf_csr(U, I, mean_log=3.0, sigma_log=0.8, dmin=2, dmax=400, zipf_a=0.9, seed=7)
    rs = np.random.RandomState(7)
    R = sp.csr_matrix((rs.randint(1, 6, size=indices.shape[0]).astype(np.float32), indices, indptr), shape=(U, I))
    W, Wv = ops.knn_build(ctx, R, "item", N, "cosine")
    Wh = host_w(W, Wv)
    Wc = Wh.tocsc()
    Wc.sort_indices()
    M = knn_ref.targets_matrix(R, "item")
    cols = np.sort(rs.choice(np.nonzero(np.diff(M.indptr))[0], size=64, replace=False))
    cols[:4] = np.argsort(-np.diff(M.indptr))[:4]                 # the most popular items among them
    for c, (x, v) in zip(cols, knn_ref.column_lists(M, cols, N, "cosine")):
        o = np.argsort(x)
        lo, hi = Wc.indptr[c], Wc.indptr[c + 1]
        assert np.array_equal(Wc.indices[lo:hi], x[o]), c
        assert same_bits(Wc.data[lo:hi], v[o]), c
    excl = ops.DeviceCSR(R.indptr, R.indices, I, ctx.device)
    Rd, Rv = ops.DeviceCSR(R.indptr, R.indices, I, ctx.device), ops.device_values(R.data, ctx.device)
    idx, val = ops.knn_score_topk(ctx, Rd, Rv, W, Wv, 0, U, k, excl=excl)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    users = np.sort(rs.choice(U, size=256, replace=False))
    preds = knn_ref.scores(R, Wh, "item", users)
    ei, ev = knn_ref.topk(preds, users, k, excl=(R.indptr, R.indices))
    assert np.array_equal(idx[users], ei)
    assert same_bits(val[users], ev)


def test_wide_counts_use_the_int64_accumulator(ctx):
    """max degree x max |r|^2 beyond int32: the build switches to 64-bit LDS counts and stays exact."""
    from elliot_amd import ops
    rs = np.random.RandomState(5)
    R = sp.random(300, 120, density=0.3, random_state=rs, format="csr", dtype=np.float32)
    R.data[:] = rs.randint(1, 20001, size=R.nnz)                 # 90 rows x 2e4^2 > 2^31
    R.data[:5] = 20000
    for sim in ("dot", "cosine"):
        W, Wv = ops.knn_build(ctx, R, "item", 15, sim)
        assert_w_equal(host_w(W, Wv), knn_ref.build_w(R, "item", 15, sim))


def test_int64_counts_across_the_tile_boundary(ctx):
    """10 240 users with ratings of 40 000 to 60 000: the 64-bit counts take two LDS tiles (8 192 cells each), every sampled dot
    list keeps neighbours from both tiles and values beyond int32.  45 columns of W bit-exact against the restatement."""
    from elliot_amd import ops
    rs = np.random.RandomState(5)
    tile, n, I, N = 8192, 8192 + 2048, 96, 20
    fixed = np.array([0, 1, tile - 1, tile, n - 1])
    cols = np.sort(np.concatenate([fixed, rs.choice(np.setdiff1d(np.arange(n), fixed), size=40, replace=False)]))
    deg = rs.randint(1, 4, size=n)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate([np.sort(rs.choice(I, size=d, replace=False)) for d in deg]).astype(np.int32)
    R = sp.csr_matrix((rs.randint(40000, 60001, size=indices.shape[0]).astype(np.float32), indices, indptr), shape=(n, I))
    assert float(deg.max()) * float(R.data.max()) ** 2 > 2 ** 31 - 1             # el_knn_build picks the 64-bit cells
    M = knn_ref.targets_matrix(R, "user")
    for sim in ("dot", "cosine"):
        W, Wv = ops.knn_build(ctx, R, "user", N, sim)
        Wc = host_w(W, Wv).tocsc()
        Wc.sort_indices()
        for c, (x, v) in zip(cols, knn_ref.column_lists(M, cols, N, sim)):
            if sim == "dot":
                assert len(x) == N and x.min() < tile <= x.max() and v.max() > 2.0 ** 31, c
            o = np.argsort(x)
            lo, hi = Wc.indptr[c], Wc.indptr[c + 1]
            assert np.array_equal(Wc.indices[lo:hi], x[o]), (sim, c)
            assert same_bits(Wc.data[lo:hi], v[o]), (sim, c)


def test_half_step_ratings(ctx):
    from elliot_amd import ops
    rs = np.random.RandomState(2)
    R = sp.random(200, 90, density=0.15, random_state=rs, format="csr", dtype=np.float32)
    R.data[:] = rs.randint(1, 11, size=R.nnz) / 2.0
    for side in ("item", "user"):
        W, Wv = ops.knn_build(ctx, R, side, 12, "cosine")
        assert_w_equal(host_w(W, Wv), knn_ref.build_w(R, side, 12, "cosine"))


def test_deterministic_bytes(ctx, golden):
    from elliot_amd import ops
    _, R = fixture_matrix(golden, "user", False)
    outs = []
    for _ in range(2):
        W, Wv = ops.knn_build(ctx, R, "user", 20, "cosine")
        Rd, Rv = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], ctx.device), ops.device_values(R.data, ctx.device)
        idx, val = ops.knn_score_topk(ctx, W, Wv, Rd, Rv, 0, R.shape[0], 10, excl=Rd)
        outs.append([t.cpu().numpy().tobytes() for t in (W.indptr, W.indices, Wv, idx, val)])
    assert outs[0] == outs[1]


def test_unsupported_input_is_an_error(ctx, golden):
    from elliot_amd import _lib, ops
    _, R = fixture_matrix(golden, "item", False)
    bad = R.copy()
    bad.data[0] = 1.3
    with pytest.raises(ValueError, match="half-step"):
        ops.knn_build(ctx, bad, "item", 20, "cosine")
    with pytest.raises(ValueError, match="supported"):
        ops.knn_build(ctx, R, "item", 20, "jaccard")
    # the C entry point refuses a scale outside {1, 2} and an unknown similarity
    n = R.shape[1]
    Rt = R.T.tocsr()
    P = ops.DeviceCSR(Rt.indptr, Rt.indices, R.shape[0], ctx.device)
    Q = ops.DeviceCSR(R.indptr, R.indices, n, ctx.device)
    pv = torch.from_numpy(Rt.data.astype(np.int32)).to(ctx.device)
    qv = torch.from_numpy(R.data.astype(np.int32)).to(ctx.device)
    need = int(ctx.lib.el_knn_ws_bytes(n, 20))
    ws = torch.empty(need, dtype=torch.uint8, device=ctx.device)
    wp = torch.empty(n + 1, dtype=torch.int64, device=ctx.device)
    wi = torch.empty(n * 20, dtype=torch.int32, device=ctx.device)
    wv = torch.empty(n * 20, dtype=torch.float32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for sim, scale in ((_lib.EL_KNN_COSINE, 3), (7, 1)):
        rc = ctx.lib.el_knn_build(ctx.handle, ctx.stream(), p(P.indptr), p(P.indices), p(pv), p(Q.indptr), p(Q.indices), p(qv),
                                  n, R.shape[0], 20, sim, scale, 60, 5, p(wp), p(wi), p(wv), p(ws), need)
        assert rc != 0 and ctx.lib.el_last_error()
