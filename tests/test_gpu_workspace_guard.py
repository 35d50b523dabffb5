"""A call that is given exactly the bytes its *_ws_bytes query names stays inside them.

ops.workspace -- the one function every workspace request goes through -- is replaced by an allocator that hands out the middle
of a tensor filled with 0xA5, exactly `need` bytes long, between two 4096-byte bands (never a cached tensor).  After the operation
both bands of every allocation must be untouched, the results must be the bytes of the same call made without the patch, and at
least one guarded allocation must have been made (a call site that went round ops.workspace would otherwise pass unseen).
One small case per workspace layout: every buffer of the layout non-empty, the last one not a multiple of 256 bytes."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from elliot_amd.evaluation.evaluator import Evaluator
from elliot_amd.recommender.masks import device_masks
from tests.gpu_util import random_excl
from tests.helpers import beyond_ref

pytestmark = pytest.mark.gpu
BAND = 4096                      # a multiple of 256: the slice is aligned like the allocation


class Guard:
    def __init__(self):
        self.allocs = []

    def __call__(self, holder, attr, need, device):
        need = max(int(need), 1)
        raw = torch.full((need + 2 * BAND,), 0xA5, dtype=torch.uint8, device=device)
        self.allocs.append((raw, need))
        return raw[BAND:BAND + need]

    def check(self):
        torch.cuda.synchronize()
        assert self.allocs, "no workspace was requested through ops.workspace"
        for n, (raw, need) in enumerate(self.allocs):
            assert bool((raw[:BAND] == 0xA5).all()), f"allocation {n} ({need} bytes): written in front of the workspace"
            assert bool((raw[BAND + need:] == 0xA5).all()), f"allocation {n} ({need} bytes): written behind the workspace"


def flat(out):
    """Every tensor of a result (tensors, DeviceCSRs, tuples of them) as host bytes."""
    if isinstance(out, torch.Tensor):
        return [out.cpu().numpy().tobytes()]
    if isinstance(out, ops.DeviceCSR):
        return flat((out.indptr, out.indices))
    return [b for o in out for b in flat(o)]


def guarded(monkeypatch, run):
    """run() without the patch, then with it: the same bytes, the bands untouched."""
    plain = flat(run())
    torch.cuda.synchronize()
    guard = Guard()
    with monkeypatch.context() as m:
        m.setattr(ops, "workspace", guard)
        got = flat(run())
        guard.check()
    assert len(got) == len(plain) and all(a == b for a, b in zip(got, plain))
    return guard


def ratings(U, I, density, seed):
    rs = np.random.RandomState(seed)
    R = sp.random(U, I, density=density, random_state=rs, format="csr", dtype=np.float32)
    R.data[:] = rs.randint(1, 6, R.nnz).astype(np.float32)
    return R


@pytest.mark.parametrize("n_neighbors", [7, 400])                # 400: N is clamped to the 301 items
def test_knn_build(ctx, monkeypatch, n_neighbors):
    R = ratings(90, 301, 0.08, 1)
    guarded(monkeypatch, lambda: ops.knn_build(ctx, R, "item", n_neighbors, "cosine"))


@pytest.mark.parametrize("normalize", [True, False])
def test_rp3_rows_and_cut(ctx, monkeypatch, normalize):
    operands = ops.rp3_operands(ctx, ratings(90, 301, 0.08, 2), 0.8, 0.6)

    def run():
        idx, val, cnt = ops.rp3_rows(ctx, *operands, 7)
        return idx, val, cnt, ops.rp3_cut(ctx, idx, val, cnt, 7, normalize)
    assert len(guarded(monkeypatch, run).allocs) == 2


@pytest.mark.parametrize("exclusion", ["column", "reference"])
def test_slim_fit_and_w(ctx, monkeypatch, exclusion):
    I = 150
    csc, vals = ops.slim_csc(ctx, ratings(200, I, 0.1, 3))
    order = ops.slim_order(ctx, ops.slim_seed_state(42), I, ops.SLIM_MAX_ITER * I)

    def run():
        four = ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 7, 33, 37, exclusion=exclusion)         # 4 targets
        idx, val, cnt, n_iter = ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 7, exclusion=exclusion)
        return four, idx, val, cnt, n_iter, ops.slim_w(ctx, idx, val, cnt)
    assert len(guarded(monkeypatch, run).allocs) == 3


@pytest.mark.parametrize("U", [38000, 41000])
def test_slim_fit_wide(ctx, monkeypatch, U):
    """The residual of a target (4 U bytes) beside its 60 weights: 38 000 users still fit the 160 KiB of LDS (152 240 bytes), 41 000
    (164 240 bytes) take the global-memory placement, whose residuals and coefficients are the last two buffers of the workspace."""
    I = 60
    per_target = int(ctx.lib.el_slim_ws_bytes(U, I, 2, 7)) - int(ctx.lib.el_slim_ws_bytes(U, I, 1, 7))
    assert (per_target >= 4 * U) == (U == 41000)
    csc, vals = ops.slim_csc(ctx, ratings(U, I, 0.02, 4))
    order = ops.slim_order(ctx, ops.slim_seed_state(42), I, ops.SLIM_MAX_ITER * I)
    guarded(monkeypatch, lambda: ops.slim_fit(ctx, csc, vals, 0.01, 0.1, order, 7, 11, 15))


def test_psvd_orth(ctx, monkeypatch):
    Y0 = torch.from_numpy(np.random.RandomState(5).normal(size=(1001, 13))).to(ctx.device)

    def run():
        Y = Y0.clone()
        return Y, ops.psvd_orth(ctx, Y)
    guarded(monkeypatch, run)


def test_mt_replay_sampler(ctx, monkeypatch, golden):
    g = golden("sampler_ref.npz")
    U, I = int(g["n_users"]), int(g["n_items"])
    lp, li = g["lists_indptr"], g["lists_items"]
    lists = [li[lp[u]:lp[u + 1]].tolist() for u in range(U)]
    pos = ops.DeviceCSR(g["indptr"], g["indices"], I, ctx.device)
    guarded(monkeypatch, lambda: ops.MtReplaySampler(ctx, lists, pos, seed=42).sample(1000))


def metric_case(ctx, U=257, I=301, k=10):
    train, test, lists = beyond_ref.random_case(U, I, k, seed=6)
    data = beyond_ref.Data(U, I, train, test, k, [k], 2.0, list(ops.BEYOND_METRIC_NAMES))
    ev = Evaluator(data, None)
    idx = torch.from_numpy(np.ascontiguousarray(lists, dtype=np.int32)).to(ctx.device)
    return data, ev, ev.device_sets(data, ctx.device)["test"], idx


def test_rec_metrics(ctx, monkeypatch):
    _, _, test, idx = metric_case(ctx)
    guarded(monkeypatch, lambda: ops.rec_metrics(ctx, idx, test, 2.0, 10))                 # (no per-user rows: they live in the workspace)


def test_beyond_metrics_and_hist_finish(ctx, monkeypatch):
    data, ev, test, idx = metric_case(ctx)
    train = device_masks(data, ctx).train
    tables = ops.DeviceItemTables(ev.item_tables(data), ctx.device)

    def run():
        sums, hist = ops.beyond_metrics(ctx, idx, test, train, tables, 2.0, 10)
        stats, nov = ops.beyond_hist_finish(ctx, hist)
        return sums, hist, stats, nov, ops.beyond_entropy(ctx, idx, test, nov, 10)
    assert len(guarded(monkeypatch, run).allocs) == 3


@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_lightgcn_propagate(ctx, monkeypatch, n_layers):
    U, I, F = 97, 61, 8
    rs = np.random.RandomState(7)
    R = sp.csr_matrix((rs.rand(U, I) < 0.1).astype(np.float32))
    ip, ix, v = ops.normalized_bipartite_laplacian(R.indptr, R.indices, U, I)
    graph = ops.GraphCSR(ctx, ip, ix, v, U, F)
    Gu, Gi = rs.normal(size=(U, F)).astype(np.float32), rs.normal(size=(I, F)).astype(np.float32)

    def run():
        st = ops.LightGcnDeviceState(ctx, Gu, Gi, graph, n_layers=n_layers)      # (the state asks for its workspace when it is built)
        st.propagate()
        return st.Gu, st.Gi
    guarded(monkeypatch, run)


@pytest.mark.parametrize("route", ["screened", "list_scratch"])
def test_score_topk_screened(ctx, monkeypatch, route):
    """list_scratch: every item the same, so every score of a user ties and every user is flagged -- the exact fallback
    (el_topk_run_list) works on its scratch inside the workspace: dense tier for 64 users, item-split tier for the last one."""
    U, I, F, k = 65, 5001, 64, 10
    rs = np.random.RandomState(8)
    Gu = rs.normal(scale=0.1, size=(U, F)).astype(np.float32)
    Gi = rs.normal(scale=0.1, size=(I, F)).astype(np.float32)
    if route == "list_scratch":
        Gi[:] = Gi[0]
    t = [torch.from_numpy(a).to(ctx.device) for a in (Gu, Gi, rs.normal(scale=0.01, size=I).astype(np.float32))]
    if route == "list_scratch":
        t[2].zero_()
    indptr, indices = random_excl(rs, U, I, 0, 30)
    excl = ops.DeviceCSR(indptr, indices, I, ctx.device)

    def run():
        out = ops.score_topk(ctx, *t, 0, U, k, excl=excl, algo="screen")
        if route == "list_scratch":
            assert ops.topk_screen_stats(ctx)["fallback_users"] == U
        return out
    guarded(monkeypatch, run)
