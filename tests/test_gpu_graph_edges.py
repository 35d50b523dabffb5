"""GPU: the graph kernels (elliot_amd/csrc/el_graph.hip) at their edges, against the plain restatements of tests/helpers/graph_ref.py.
  k_spmm_csr / k_spmm_finish     a hand-built CSR with a row on every boundary of the three nested strides (4 gathers, lpt, 512) and 8, 9,
                                 10, 16 and 17 partials, on values for which fp32 is exact: the product equals SciPy's bit for bit
  el_lightgcn_propagate          1 .. 16 layers at F = 12 / 64 / 100 against fp64, independent of what its buffers held before
  k_ngcf_pre / k_ngcf_post       bitwise against one-rounding NumPy; the normalised block against fp64; the dropout mask against the host
                                 Philox, entry for entry
  k_adam_l2_dense                five steps against the fp32 and fp64 restatements of the oracle's dense Adam
  NGCFModel / LightGCNModel      a run resumed from save_weights equals the uninterrupted one bit for bit; widths the kernels cannot take
                                 are refused at construction
"""
import ctypes as C
import functools
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from elliot_amd._lib import ElliotHipError
from oracle import lightgcn as ol
from tests.gpu_util import cpu
from tests.helpers import graph_ref as gr

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float("nan")
N_EDGE = 9000


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- 1. SpMM ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _edge():
    indptr, indices, where = gr.edge_csr(N_EDGE, seed=0)
    return indptr, indices, gr.exact_vals(len(indices), np.random.RandomState(1)), where


def _edge_graph(ctx, n0, width, vals=None):
    indptr, indices, v, _ = _edge()
    g = ops.GraphCSR(ctx, indptr, indices, v if vals is None else vals, n0, width)
    cnt = set(cpu(g.multi_cnt).tolist())
    assert {8, 9, 10, 16, 17} <= cnt, cnt                         # the second trip of k_spmm_finish's loop, with and without a tail
    assert int(cpu(g.multi_row)[0]) == 0 and int(cpu(g.multi_row)[-1]) == N_EDGE - 1
    return g


def _spmm_twice(ctx, g, X):
    """[Y0; Y1] of two calls, each on a partial buffer full of NaN."""
    X0, X1 = _dev(ctx, X[:g.n0]), _dev(ctx, X[g.n0:])
    out = []
    for _ in range(2):
        g.part.fill_(NAN)
        Y0, Y1 = g.spmm(X0, X1)
        out.append(np.concatenate([cpu(Y0), cpu(Y1)]))
    return out


def _assert_exact_product(ctx, g, F, seed):
    indptr, indices, vals, _ = _edge()
    X = gr.exact_table(N_EDGE, F, np.random.RandomState(seed))
    ref64 = gr.spmm_f64(indptr, indices, vals, X)
    ref = ref64.astype(f32)
    assert np.abs(ref64).max() < 2 ** 18 and np.array_equal(ref.astype(np.float64), ref64)       # the reference itself is exact in fp32
    got, again = _spmm_twice(ctx, g, X)
    if not np.array_equal(_bits(got), _bits(ref)):
        bad = np.nonzero((got != ref).any(1))[0]
        lens = np.diff(indptr)[bad]
        raise AssertionError(f"F={F} n0={g.n0}: {len(bad)} rows differ from the exact product; rows {bad[:12].tolist()} of lengths "
                             f"{lens[:12].tolist()}; first: got {got[bad[0]][:4].tolist()} want {ref[bad[0]][:4].tolist()}")
    assert np.array_equal(_bits(got), _bits(again)), "a second call gave other bits"


# F -> (lpt, CPL) of el_pick_lpt(F, 4) + spmm_launch: lpt = the power of two in [8, 64] that first covers F / 4 vectors, CPL = 1, 2 or 4
# vectors per lane once lpt = 64 is not enough.  CPL > 1 exists only with lpt = 64, so these are all six pairs the launcher can reach.
@pytest.mark.parametrize("F", [
    4,      # (8, 1)   one live lane of eight
    8,      # (8, 1)
    12,     # (8, 1)
    20,     # (8, 1)
    36,     # (16, 1)  9 of 16 lanes live
    68,     # (32, 1)  17 of 32
    100,    # (32, 1)  25 of 32
    132,    # (64, 1)  33 of 64
    260,    # (64, 2)  the second slice holds one live lane
    516,    # (64, 4)  three slices' worth: the third holds one live lane, the fourth none
    1024,   # (64, 4)  every lane of every slice
])
def test_spmm_is_exact_on_every_stride_boundary(ctx, F):
    """Rows of every length in graph_ref.ROW_LENGTHS (0 .. 8 197 non-zeros: 1 .. 17 partials), rows 0 and N - 1 cut into chunks,
    n0 in the middle with multi-chunk rows on both sides: the product of exactly representable values equals SciPy's fp64 product
    bit for bit, whatever `part` held before, twice."""
    _, _, _, where = _edge()
    assert all(n in where for n in gr.ROW_LENGTHS)
    _assert_exact_product(ctx, _edge_graph(ctx, N_EDGE // 2, F), F, seed=F)


@pytest.mark.parametrize("n0", [1, N_EDGE - 1])
@pytest.mark.parametrize("F", [12, 100, 516])
def test_spmm_is_exact_with_the_table_split_next_to_either_end(ctx, F, n0):
    _assert_exact_product(ctx, _edge_graph(ctx, n0, F), F, seed=F + n0)


def test_spmm_graph_sized_for_a_wider_table_serves_a_narrower_one(ctx):
    """What NGCF always does: `part` is strided by the F of the call, not by the graph's width."""
    g = _edge_graph(ctx, N_EDGE // 2, 64)
    _assert_exact_product(ctx, g, 12, seed=3)
    _assert_exact_product(ctx, g, 64, seed=4)


@pytest.mark.parametrize("n0", [0, N_EDGE])
def test_spmm_with_one_table_empty_gives_the_exact_product(ctx, n0):
    """el_spmm_csr_f32 defines both: with n0 == N no row index resolves into the second table, with n0 == 0 none into the first, and
    the half without rows may be a null pointer (a zero-row torch tensor's is).  The product is the exact one."""
    _assert_exact_product(ctx, _edge_graph(ctx, n0, 20), 20, seed=n0 + 5)


def test_spmm_random_values_on_the_edge_structure(ctx):
    """The existing random test's bound, 4e-7 * mag + 1e-12, on this structure at F = 100 (tests/test_graph_ref.py shows on the CPU that a
    fp32 sum in the kernels' order keeps it)."""
    indptr, indices, _, _ = _edge()
    rs = np.random.RandomState(11)
    vals = rs.normal(size=len(indices)).astype(f32)
    X = rs.normal(size=(N_EDGE, 100)).astype(f32)
    g = _edge_graph(ctx, N_EDGE // 2, 100, vals)
    got, again = _spmm_twice(ctx, g, X)
    ref, mag = gr.spmm_f64(indptr, indices, vals, X), gr.spmm_magnitude(indptr, indices, vals, X)
    excess = np.abs(got - ref) - (4e-7 * mag + 1e-12)
    assert (excess <= 0).all(), (float(excess.max()), np.diff(indptr)[np.nonzero((excess > 0).any(1))[0]][:10].tolist())
    assert np.array_equal(_bits(got), _bits(again))
    # the kernels add a chunk's terms in sequence and a row's partials in order, without contraction: the bits of that fp32 sum
    assert np.array_equal(_bits(got), _bits(gr.spmm_chunk_order_f32(indptr, indices, vals, X)))


@pytest.mark.parametrize("F", [2, 10, 1028])
def test_spmm_refuses_widths_it_cannot_vectorise(ctx, F):
    indptr, indices = np.arange(0, 18, 2, dtype=np.int64), np.tile(np.asarray([1, 5], np.int32), 8)
    g = ops.GraphCSR(ctx, indptr, indices, np.ones(16, f32), 3, 1028)
    X0, X1 = torch.zeros((3, F), device=ctx.device), torch.zeros((5, F), device=ctx.device)
    with pytest.raises(ElliotHipError, match="multiples of 4"):
        g.spmm(X0, X1)


# ---- 2. LightGCN propagation --------------------------------------------------------------------------------------------------------
LG_U, LG_I, LG_LONELY_USER, LG_LONELY_ITEM = 5000, 60, 7, 59


@functools.lru_cache(None)
def _lgcn():
    rs = np.random.RandomState(2)
    dense = rs.rand(LG_U, LG_I) < 0.05
    dense[:, 0] = True                                            # item 0: every user but the isolated one -- 4 999 neighbours, 10 partials
    dense[:, LG_LONELY_ITEM] = False
    dense[LG_LONELY_USER, :] = False
    R = sp.csr_matrix(dense.astype(f32))
    ip, ix, v = ops.normalized_bipartite_laplacian(R.indptr, R.indices, LG_U, LG_I)
    return ip, ix, v, sp.csr_matrix((v, ix, ip), shape=(LG_U + LG_I,) * 2)


def _err(got, ref):
    return max(float(np.abs(got[0] - ref[0]).max()), float(np.abs(got[1] - ref[1]).max()))


@pytest.mark.parametrize("F", [12, 64, 100])
@pytest.mark.parametrize("n_layers", [1, 2, 3, 5, 6, 16])
def test_lightgcn_propagate_deep_stacks_against_fp64(ctx, n_layers, F):
    """el_lightgcn_propagate against the fp64 restatement of LightGCN_model.py:68-94.  Bound: max(2e-6, 4 e_o) with e_o the error of the
    fp32 NumPy oracle (oracle/lightgcn.py: propagate) against the same fp64 -- 2e-6 is the existing test's bound at this table scale, the
    factor 4 allows another (fixed) summation order.  The result does not depend on what the workspace and the partial buffer held
    (NaN here), a second call equals the restatement applied twice, and isolated nodes come out as x / (n_layers + 1) exactly."""
    ip, ix, v, L = _lgcn()
    rs = np.random.RandomState(100 * n_layers + F)
    Gu = rs.normal(scale=0.3, size=(LG_U, F)).astype(f32)
    Gi = rs.normal(scale=0.3, size=(LG_I, F)).astype(f32)
    g = ops.GraphCSR(ctx, ip, ix, v, LG_U, F)
    assert 10 in cpu(g.multi_cnt).tolist()
    ref = gr.lightgcn_propagate_f64(Gu, Gi, L, n_layers)
    orc = ol.propagate(Gu, Gi, L, n_layers)
    e_o = _err(orc, ref)
    fresh = ops.LightGcnDeviceState(ctx, Gu, Gi, g, n_layers=n_layers)
    fresh.propagate()
    A = cpu(fresh.Gu), cpu(fresh.Gi)
    assert _err(A, ref) <= max(2e-6, 4 * e_o), f"kernel error {_err(A, ref):.3e}, oracle error e_o {e_o:.3e}"
    d = f32(n_layers + 1)
    assert np.array_equal(_bits(A[0][LG_LONELY_USER]), _bits(Gu[LG_LONELY_USER] / d))
    assert np.array_equal(_bits(A[1][LG_LONELY_ITEM]), _bits(Gi[LG_LONELY_ITEM] / d))
    st = ops.LightGcnDeviceState(ctx, Gu, Gi, g, n_layers=n_layers)
    st._ws.view(torch.float32).fill_(NAN)
    g.part.fill_(NAN)
    st.propagate()
    B = cpu(st.Gu), cpu(st.Gi)
    assert not np.isnan(B[0]).any() and not np.isnan(B[1]).any()
    assert np.array_equal(_bits(A[0]), _bits(B[0])) and np.array_equal(_bits(A[1]), _bits(B[1]))
    st.propagate()
    ref2 = gr.lightgcn_propagate_f64(ref[0], ref[1], L, n_layers)
    e_o2 = _err(ol.propagate(orc[0], orc[1], L, n_layers), ref2)
    err2 = _err((cpu(st.Gu), cpu(st.Gi)), ref2)
    assert err2 <= max(2e-6, 4 * e_o2), f"second call: kernel error {err2:.3e}, oracle error e_o {e_o2:.3e}"


def test_lightgcn_propagate_refuses_17_layers(ctx):
    ip, ix, v, _ = _lgcn()
    Gu, Gi = np.ones((LG_U, 12), f32), np.ones((LG_I, 12), f32)
    st = ops.LightGcnDeviceState(ctx, Gu, Gi, ops.GraphCSR(ctx, ip, ix, v, LG_U, 12), n_layers=17)
    with pytest.raises(ElliotHipError, match="el_lightgcn_propagate"):
        st.propagate()
    assert np.array_equal(cpu(st.Gu), Gu) and np.array_equal(cpu(st.Gi), Gi)


# ---- 3. NGCF: the dense half --------------------------------------------------------------------------------------------------------
def _ngcf_pre(ctx, ego, lap, N, k, X2):
    return ctx.lib.el_ngcf_pre(ctx.handle, ctx.stream(), ops._ptr(ego), ops._ptr(lap), N, k, ops._ptr(X2))


def test_ngcf_pre_equals_one_rounding_per_element(ctx):
    rs = np.random.RandomState(3)
    for N in (1, 257):
        for k in (4, 12, 64, 100):
            ego, lap = rs.normal(size=(N, k)).astype(f32), rs.normal(size=(N, k)).astype(f32)
            X2 = torch.full((N, 2 * k), NAN, device=ctx.device)
            ops.check(_ngcf_pre(ctx, _dev(ctx, ego), _dev(ctx, lap), N, k, X2), "el_ngcf_pre")
            assert np.array_equal(_bits(cpu(X2)), _bits(gr.ngcf_pre(ego, lap))), (N, k)
    one = torch.ones((1, 12), device=ctx.device)
    X2 = torch.full((1, 24), -7.25, device=ctx.device)
    assert _ngcf_pre(ctx, one, one, 0, 12, X2) == 0 and bool((X2 == -7.25).all())              # no rows: success, nothing written
    with pytest.raises(ElliotHipError, match="multiple of 4"):
        ops.check(_ngcf_pre(ctx, one, one, 1, 10, X2), "el_ngcf_pre")


SENTINEL = f32(-7.25)


def _ngcf_post(ctx, S, n0, W, col_off, rate=0.0, seed=42, step=0):
    """el_ngcf_post on sentinel-filled tables (one guard row behind each, a guard tail behind ego_next) -> (ego_next, the stacked
    [Gu; Gi] rows); the guards are checked here."""
    N, kout = S.shape
    Gu = torch.full((n0 + 1, W), float(SENTINEL), device=ctx.device)
    Gi = torch.full((N - n0 + 1, W), float(SENTINEL), device=ctx.device)
    ego = torch.full((N * kout + 64,), float(SENTINEL), device=ctx.device)
    ops.check(ctx.lib.el_ngcf_post(ctx.handle, ctx.stream(), ops._ptr(_dev(ctx, S)), N, n0, kout, float(rate), seed, step, ops._ptr(ego),
                                   ops._ptr(Gu), ops._ptr(Gi), W, col_off), "el_ngcf_post")
    Gu, Gi, ego = cpu(Gu), cpu(Gi), cpu(ego)
    assert (Gu[n0] == SENTINEL).all() and (Gi[N - n0] == SENTINEL).all() and (ego[N * kout:] == SENTINEL).all()
    return ego[:N * kout].reshape(N, kout), np.concatenate([Gu[:n0], Gi[:N - n0]])


def _assert_normalised_block(G, ego, col_off, what):
    """Columns outside [col_off, col_off + kout) keep the sentinel; the block is ego / sqrt(max(sum ego^2, 1e-12)) within
    2e-6 * max |ref row|: at most (kout / 64 + 8) roundings of 2^-24 in the sum, the reciprocal square root and the product."""
    kout = ego.shape[1]
    out = np.delete(G, np.s_[col_off:col_off + kout], axis=1)
    assert np.array_equal(_bits(out), _bits(np.full_like(out, SENTINEL))), what
    ref = gr.l2_normalize_f64(ego)
    tol = 2e-6 * np.abs(ref).max(1, keepdims=True)
    assert (np.abs(G[:, col_off:col_off + kout] - ref) <= tol).all(), what


@pytest.mark.parametrize("N", [1, 5, 4099])
def test_ngcf_post_without_dropout(ctx, N):
    """One wave per row, four rows per workgroup: kout on both sides of the 64-lane stride, n0 at 0, inside the first workgroup's four
    rows and at N, a block in the middle of a wider row -- ego_next bitwise, the block against fp64, everything else untouched; an
    all-zero row gives 0 (not NaN), a row with sum x^2 < 1e-12 gives x * 1e6."""
    rs = np.random.RandomState(N)
    for kout in (1, 8, 63, 64, 65, 200):
        S = rs.normal(size=(N, kout)).astype(f32)
        if N >= 5:
            S[1] = 0.0
            S[3] = (1e-8 * rs.choice([-1.0, 1.0], kout)).astype(f32)
        want = gr.leaky_relu(S)
        for n0 in sorted({0, min(2, N), N}):
            for col_off in (0, 5):
                what = (N, kout, n0, col_off)
                ego, G = _ngcf_post(ctx, S, n0, col_off + kout + 3, col_off)
                assert np.array_equal(_bits(ego), _bits(want)), what
                _assert_normalised_block(G, want, col_off, what)
                if N >= 5:
                    blk = G[:, col_off:col_off + kout]
                    assert not blk[1].any(), what
                    assert (np.abs(blk[3] - want[3].astype(np.float64) * 1e6) <= 2e-6 * np.abs(want[3]).max() * 1e6).all(), what


def test_ngcf_post_dropout_mask_equals_the_host_philox(ctx):
    """Rate 0.3 at N = 37, kout = 70: the zero pattern is the restated mask (graph_ref.dropout_keep) entry for entry, the kept entries
    are leaky_relu(s) * fl32(1 / (1 - rate)) bit for bit."""
    N, kout, n0, rate, seed, step = 37, 70, 20, 0.3, 0x9E3779B97F4A7C15, 16 * 5 + 1
    rs = np.random.RandomState(7)
    S = (rs.choice([-1.0, 1.0], (N, kout)) * rs.uniform(0.05, 2.0, (N, kout))).astype(f32)
    ego, G = _ngcf_post(ctx, S, n0, kout + 8, 5, rate=rate, seed=seed, step=step)
    keep = gr.dropout_keep(N, kout, rate, seed, step)
    assert 0.15 < 1 - keep.mean() < 0.45                                                         # (the restatement itself drops something)
    assert np.array_equal(ego == 0, ~keep)
    scale = f32(1.0) / (f32(1.0) - f32(rate))
    want = np.where(keep, gr.leaky_relu(S) * scale, f32(0.0)).astype(f32)
    assert np.array_equal(_bits(ego), _bits(want))
    _assert_normalised_block(G, want, 5, "dropout")


def test_ngcf_post_dropout_statistics_and_refusals(ctx):
    """262 144 Bernoulli(0.3) draws: the dropped share within six standard deviations overall (0.006) and per column (0.043 of 4 096
    draws); rows do not repeat their neighbour's mask; (seed, step) fixes the bits, either one changes them; rates outside [0, 1) are
    refused."""
    N, kout, rate = 4096, 64, 0.3
    S = np.random.RandomState(9).uniform(0.5, 1.5, (N, kout)).astype(f32)
    run = lambda seed, step: _ngcf_post(ctx, S, 1000, kout, 0, rate=rate, seed=seed, step=step)[0]
    ego = run(42, 3)
    drop = ego == 0
    assert abs(drop.mean() - rate) <= 0.006, drop.mean()
    assert np.abs(drop.mean(0) - rate).max() <= 0.043, drop.mean(0)
    assert (drop[1:] != drop[:-1]).any(1).all()
    assert np.array_equal(_bits(run(42, 3)), _bits(ego))
    assert not np.array_equal(run(42, 4) == 0, drop) and not np.array_equal(run(43, 3) == 0, drop)
    for bad in (1.0, -0.1):
        with pytest.raises(ElliotHipError, match="dropout rate"):
            _ngcf_post(ctx, S[:4], 2, kout, 0, rate=bad)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_adam_l2_dense_against_the_oracles_dense_adam(ctx, n):
    """Five steps, each started from the fp32 restatement's own state (NGCFOracle.train_step's GraphLayers update, restated in
    graph_ref.adam_l2_dense).  theta, m and v differ from the fp32 restatement by at most 4 * 2^-23 * max(|ref|, |update|) -- the three
    multiply-adds may be contracted, one ulp each -- and from fp64 by at most 4 times the fp32 restatement's own error, with that floor.
    theta = 0 stays 0 with m = v = 0."""
    rs = np.random.RandomState(n)
    lr, two_lw = 0.005, 2.0 * 0.02
    th = rs.normal(scale=0.3, size=n).astype(f32)
    th[::7] = 0.0
    m, v = np.zeros(n, f32), np.zeros(n, f32)
    ulp4 = 4 * 2.0 ** -23
    for t in range(1, 6):
        lr_t = ops.adam_lr_t(lr, t)
        d = [_dev(ctx, x) for x in (th, m, v)]
        ops.check(ctx.lib.el_adam_l2_dense(ctx.handle, ctx.stream(), *(ops._ptr(x) for x in d), n, C.c_float(lr_t), C.c_float(two_lw)),
                  "el_adam_l2_dense")
        got = [cpu(x) for x in d]
        r32 = gr.adam_l2_dense(th, m, v, lr_t, two_lw, np.float32)
        r64 = gr.adam_l2_dense(th, m, v, lr_t, two_lw, np.float64)
        for name, x, a, b, up in zip(("theta", "m", "v"), got, r32[:3], r64[:3], r32[3]):
            assert not np.isnan(x).any(), (name, t)
            floor = ulp4 * np.maximum(np.abs(a), np.abs(up)).astype(np.float64)
            assert (np.abs(x.astype(np.float64) - a) <= floor).all(), (name, t, float(np.abs(x - a).max()))
            e_rest = float(np.abs(a - b).max())
            assert (np.abs(x - b) <= np.maximum(floor, 4 * e_rest)).all(), (name, t, float(np.abs(x - b).max()), e_rest)
        assert not got[0][::7].any() and not got[1][::7].any() and not got[2][::7].any(), t
        th, m, v = r32[:3]


# ---- 4. resume and early refusal ----------------------------------------------------------------------------------------------------
RS_U, RS_I, RS_K, RS_WS, RS_B = 1024, 50, 8, (12, 8), 2048


@functools.lru_cache(None)
def _small_laplacian():
    R = sp.random(RS_U, RS_I, density=0.12, format="csr", random_state=np.random.RandomState(4), dtype=f32)
    ip, ix, v = ops.normalized_bipartite_laplacian(R.indptr, R.indices, RS_U, RS_I)
    return sp.csr_matrix((v, ix, ip), shape=(RS_U + RS_I,) * 2)


def _batches(n):
    """Fixed triplets in which every user occurs exactly twice.  On tables this small the sorted BPR step adds the pieces of a user
    segment that chunk boundaries (every 4 sorted positions) cut into a dense accumulator with float atomics: up to two pieces commute,
    three or more would make the last bit depend on the launch -- and "bit for bit" below is about the restored state, not about that."""
    rs = np.random.RandomState(6)
    return [(np.concatenate([rs.permutation(RS_U), rs.permutation(RS_U)]), rs.randint(0, RS_I, RS_B), rs.randint(0, RS_I, RS_B))
            for _ in range(n)]


def _ngcf_weights(seed):
    rs = np.random.RandomState(seed)
    sizes = (RS_K,) + RS_WS
    W = sum(sizes)
    Gu, Gi = np.zeros((RS_U, W), f32), np.zeros((RS_I, W), f32)
    Gu[:, :RS_K], Gi[:, :RS_K] = rs.normal(scale=0.2, size=(RS_U, RS_K)), rs.normal(scale=0.2, size=(RS_I, RS_K))
    layers = [{"W1": rs.normal(scale=0.3, size=(a, b)).astype(f32), "b1": rs.normal(scale=0.1, size=(1, b)).astype(f32),
               "W2": rs.normal(scale=0.3, size=(a, b)).astype(f32), "b2": rs.normal(scale=0.1, size=(1, b)).astype(f32)}
              for a, b in zip(sizes[:-1], sizes[1:])]
    return Gu, Gi, layers


def _ngcf(ctx, weights, dropout=(0.0, 0.0), embed_k=RS_K, weight_size=RS_WS):
    from elliot_amd.recommender.graph_based.ngcf.NGCF_model import NGCFModel
    return NGCFModel(num_users=RS_U, num_items=RS_I, learning_rate=0.005, embed_k=embed_k, l_w=0.02, weight_size=weight_size,
                     n_layers=len(weight_size), node_dropout=(), message_dropout=dropout, n_fold=1, adjacency=None,
                     laplacian=_small_laplacian(), random_seed=42, ctx=ctx, init_weights=weights)


def _lightgcn(ctx, weights, embed_k=RS_K):
    from elliot_amd.recommender.graph_based.lightgcn.LightGCN_model import LightGCNModel
    return LightGCNModel(num_users=RS_U, num_items=RS_I, learning_rate=0.005, embed_k=embed_k, l_w=0.02, n_layers=2, n_fold=1,
                         adjacency=None, laplacian=_small_laplacian(), random_seed=42, ctx=ctx, init_weights=weights)


def _lightgcn_weights(seed):
    rs = np.random.RandomState(seed)
    return rs.normal(scale=0.2, size=(RS_U, RS_K)).astype(f32), rs.normal(scale=0.2, size=(RS_I, RS_K)).astype(f32)


def _params(model):
    """Every trained array of a model, by name."""
    st = model.state
    out = {"Gu": cpu(st.Gu), "Gi": cpu(st.Gi)}
    for k, l in enumerate(getattr(st, "layers", [])):
        out.update({f"layer{k}.{name}": cpu(p) for name, p in l.items()})
    return out


def _assert_same_bits(got, want):
    assert got.keys() == want.keys()
    for name in want:
        assert np.array_equal(_bits(got[name]), _bits(want[name])), \
            f"{name}: the resumed run differs from the uninterrupted one (max |diff| {np.abs(got[name] - want[name]).max():.3e})"


def _assert_resume(make, first, second, path):
    """Two steps, save, a third step -- against a second model (built on other weights) that loads the file and takes the third step."""
    b = _batches(3)
    one = make(first)
    one.train_step(b[0])
    one.train_step(b[1])
    one.save_weights(path)
    one.train_step(b[2])
    two = make(second)
    two.load_weights(path)
    assert two.state.step == 2
    two.train_step(b[2])
    _assert_same_bits(_params(two), _params(one))


@pytest.mark.parametrize("dropout", [(0.0, 0.0), (0.3, 0.0)])
def test_ngcf_resumed_run_equals_the_uninterrupted_one(ctx, tmp_path, dropout):
    """save_weights carries the tables' Adam moments, the GraphLayers' (m, v) slots and the step count (which also seeds the
    message-dropout mask): step three after a load equals step three of the run that never stopped, bit for bit."""
    _assert_resume(lambda w: _ngcf(ctx, w, dropout), _ngcf_weights(1), _ngcf_weights(2), tmp_path / "ngcf.pkl")


def test_lightgcn_resumed_run_equals_the_uninterrupted_one(ctx, tmp_path):
    _assert_resume(lambda w: _lightgcn(ctx, w), _lightgcn_weights(1), _lightgcn_weights(2), tmp_path / "lightgcn.pkl")


@pytest.mark.parametrize("kind", ["ngcf", "lightgcn"])
def test_loading_a_state_without_moments_restarts_adam(ctx, tmp_path, kind):
    """An older file holds no moments: Adam restarts as a whole -- step 0 on zero moments, never the saved step on zero (or stale)
    moments -- and the next step equals the first step of a model built on the saved weights."""
    make, weights = ((lambda w: _ngcf(ctx, w)), _ngcf_weights) if kind == "ngcf" else ((lambda w: _lightgcn(ctx, w)), _lightgcn_weights)
    b = _batches(3)
    one = make(weights(1))
    one.train_step(b[0])
    one.train_step(b[1])
    old = {k: v for k, v in one.get_model_state().items() if k not in ("mGu", "vGu", "mGi", "vGi", "layer_slots")}
    assert old["_step"] == 2
    with open(tmp_path / "old.pkl", "wb") as f:
        pickle.dump(old, f)
    two = make(weights(2))
    two.train_step(b[0])                                          # moments and a step count of its own, to be discarded
    two.load_weights(tmp_path / "old.pkl")
    st = two.state
    assert st.step == 0
    assert not any(bool(getattr(st.bpr, n).any()) for n in ("mGu", "vGu", "mGi", "vGi"))
    assert not any(bool(m.any()) or bool(v.any()) for sl in getattr(st, "slots", []) for m, v in sl.values())
    two.train_step(b[2])
    new = make((old["Gu"], old["Gi"], old["layers"]) if kind == "ngcf" else (old["Gu"], old["Gi"]))
    new.train_step(b[2])
    _assert_same_bits(_params(two), _params(new))


def test_models_refuse_widths_the_kernels_cannot_take_at_construction(ctx):
    """A deviation from the reference (which accepts any width): `factors` and every `weight_size` entry must be multiples of 4, said
    by name when the model is built, not by the first train step's kernel."""
    with pytest.raises(ValueError, match=r"factors.*multiple of 4"):
        _lightgcn(ctx, None, embed_k=10)
    with pytest.raises(ValueError, match=r"factors.*multiple of 4"):
        _ngcf(ctx, None, embed_k=10)
    with pytest.raises(ValueError, match=r"weight_size.*multiple of 4"):
        _ngcf(ctx, None, weight_size=(50,))


def test_plugins_refuse_widths_the_kernels_cannot_take_at_construction(ctx, tmp_path):
    from types import SimpleNamespace

    from elliot_amd.recommender import NGCF, LightGCN
    from tests.test_gpu_plugin import make_data
    data, cfg = make_data(tmp_path)
    params = lambda **kw: SimpleNamespace(meta=SimpleNamespace(save_recs=False, verbose=False), epochs=1, batch_size=512, seed=42, **kw)
    with pytest.raises(ValueError, match=r"factors.*multiple of 4"):
        LightGCN(data=data, config=cfg, params=params(latent_dim=10))
    with pytest.raises(ValueError, match=r"factors.*multiple of 4"):
        NGCF(data=data, config=cfg, params=params(latent_dim=10))
    with pytest.raises(ValueError, match=r"weight_size.*multiple of 4"):
        NGCF(data=data, config=cfg, params=params(latent_dim=16, weight_size="(50,)"))
