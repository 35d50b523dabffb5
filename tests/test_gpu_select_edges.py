"""The one-wave selection (ElWaveSelect of csrc/el_topk_common.h) at its edges, through its two key policies: the packed fp32
key (el_dense_topk, el_score_topk on its `simple` route) and the pair key (el_dense_topk_f64, el_score_topk_f64, the RP3beta row
cut).  Every list is compared bit for bit, indices and values: dense input against a stable NumPy sort on (value desc, index asc)
with the library's padding rule, scoring input against the C oracle.

k crosses the steps of el_select_cap (64 | 65, 192 | 193), I crosses the 64 lanes of a pass; k > I and k > the number of allowed
items make the padding run.  The rows: ascending values (every pass appends 64 and a compaction runs every pass), descending
(the threshold refuses everything behind the first compaction), all equal (ties carried across compactions by index), -0.0
beside +0.0, NaN (never selected), -inf and +inf, and values that differ only below fp32 resolution."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from oracle import cref
from tests.gpu_util import cpu

gpu = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 129]
KS = [1, 63, 64, 65, 192, 193]
KINDS = ["asc", "desc", "equal", "zeros", "nan", "inf", "sub32"]
ROWS = 4                                     # rows of a scoring case (a dense case has one row per kind)
SCALES = np.array([1.0, 2.0, 0.5, 4.0])      # user factors of the F = 1 scoring rows: exact products, order and ties kept


def content(kind, I):
    """One row of values, float64."""
    j = np.arange(I, dtype=np.float64)
    rs = np.random.RandomState(I)
    if kind == "asc":
        return j * 0.5 - 3.0
    if kind == "desc":
        return 40.0 - j * 0.25
    if kind == "equal":
        return np.full(I, 1.25)
    if kind == "zeros":
        v = np.where(j % 2 == 0, -0.0, 0.0)
        v[3::7] = 1.0
        v[5::11] = -1.0
        return v
    v = np.round(rs.normal(size=I) * 8.0) / 4.0              # few distinct values: ties among the finite ones too
    if kind == "nan":
        v[0::3] = np.nan
        return v
    if kind == "inf":
        v[1::5] = np.inf
        v[0::4] = -np.inf
        return v
    assert kind == "sub32"
    return 1.0 + ((np.arange(I) * 37) % I) * 2.0 ** -40     # one float32, I doubles


def mask_rows(I, n, lo=0, extra=0):
    """n sorted rows of items for an exclusion or a candidate CSR over the items [lo, lo + I) (extra: as many items on either
    side of that range as well): none of them, all of them, all but one, and random subsets."""
    rs = np.random.RandomState(1000 + I + n)
    items = np.arange(lo - min(lo, extra), lo + I + extra)
    rows = []
    for r in range(n):
        if r % 4 == 0:
            keep = rs.rand(items.shape[0]) < 0.5
        elif r % 4 == 1:
            keep = np.ones(items.shape[0], bool)
        elif r % 4 == 2:
            keep = np.zeros(items.shape[0], bool)
        else:
            keep = np.ones(items.shape[0], bool)
            keep[rs.randint(items.shape[0])] = False
        rows.append(items[keep])
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def dense_reference(preds, k, excl=None, cand=None):
    """Stable sort on (value desc, index asc) of the allowed, non-NaN items (value + 0: -0.0 ranks and reads as +0.0); a short
    list goes on with the masked items in ascending order (the items outside the candidate row, or the excluded items), then
    with -1, all at -inf."""
    n, I = preds.shape
    idx = np.full((n, k), -1, np.int32)
    val = np.full((n, k), -np.inf, preds.dtype)
    every = np.arange(I)
    for u in range(n):
        if cand is not None:
            allowed = cand[1][cand[0][u]:cand[0][u + 1]].astype(np.int64)
            masked = np.setdiff1d(every, allowed)
        elif excl is not None:
            masked = excl[1][excl[0][u]:excl[0][u + 1]].astype(np.int64)
            allowed = np.setdiff1d(every, masked)
        else:
            allowed, masked = every, every[:0]
        v = preds[u, allowed] + preds.dtype.type(0)
        allowed, v = allowed[~np.isnan(v)], v[~np.isnan(v)]
        order = np.argsort(-v, kind="stable")[:k]
        m = order.shape[0]
        idx[u, :m], val[u, :m] = allowed[order], v[order]
        fill = masked[:k - m]
        idx[u, m:m + fill.shape[0]] = fill
    return idx, val


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def device_csr(ctx, m, n_cols):
    return None if m is None else ops.DeviceCSR(m[0], m[1], n_cols, ctx.device)


@gpu
@pytest.mark.parametrize("mode", ["none", "excl", "cand"])
@pytest.mark.parametrize("I", SIZES)
def test_dense_lists_equal_the_stable_sort(ctx, I, mode):
    n = len(KINDS)
    m = None if mode == "none" else mask_rows(I, n)
    kw = {} if m is None else {mode: m}
    dkw = {} if m is None else {mode: device_csr(ctx, m, I)}
    p64 = np.stack([content(kind, I) for kind in KINDS])
    bad = []
    for dtype, fn in ((np.float32, ops.dense_topk), (np.float64, ops.dense_topk_f64)):
        preds = p64.astype(dtype)
        dev = torch.from_numpy(preds).to(ctx.device)
        for k in KS:
            ei, ev = dense_reference(preds, k, **kw)
            gi, gv = fn(ctx, dev, 0, n, k, **dkw)
            gi, gv = cpu(gi), cpu(gv)
            for r, kind in enumerate(KINDS):
                if not (same_bits(gi[r], ei[r]) and same_bits(gv[r], ev[r])):
                    bad.append((np.dtype(dtype).name, k, kind))
    assert not bad, bad


def scoring_tables(kind, I, F):
    """Item column 0 holds the row content; F = 1: user factor a power of two.  F = 5: four random columns behind it."""
    rs = np.random.RandomState(7 * I + F)
    Q = np.concatenate([content(kind, I)[:, None], np.round(rs.normal(size=(I, F - 1)) * 16.0) / 16.0], axis=1)
    P = np.concatenate([SCALES[:ROWS, None], np.round(rs.normal(size=(ROWS, F - 1)) * 16.0) / 16.0], axis=1)
    return P, Q


def run_scoring(ctx, I, modes, item_offset=0, extra=0):
    bad = []
    for mode in modes:
        m = None if mode == "none" else mask_rows(I, ROWS, item_offset, extra)
        kw = {} if m is None else {mode: m}
        dkw = {} if m is None else {mode: device_csr(ctx, m, item_offset + I + extra)}
        for kind in KINDS:
            for F in (1, 5):
                P64, Q64 = scoring_tables(kind, I, F)
                for dtype in (np.float32, np.float64):
                    P, Q = P64.astype(dtype), Q64.astype(dtype)
                    dP, dQ = torch.from_numpy(P).to(ctx.device), torch.from_numpy(Q).to(ctx.device)
                    for k in KS:
                        if dtype == np.float32:
                            ei, ev = cref.score_topk_f32(P, Q, None, 0, ROWS, k, item_offset=item_offset, **kw)
                            gi, gv = ops.score_topk(ctx, dP, dQ, None, 0, ROWS, k, item_offset=item_offset, algo="simple", **dkw)
                        else:
                            ei, ev = cref.score_topk_f64(P, Q, None, 0, ROWS, k, item_offset=item_offset, **kw)
                            gi, gv = ops.score_topk_f64(ctx, dP, dQ, None, 0, ROWS, k, item_offset=item_offset, **dkw)
                        if not (same_bits(cpu(gi), ei) and same_bits(cpu(gv), ev)):
                            bad.append((mode, kind, F, np.dtype(dtype).name, k))
    return bad


@gpu
@pytest.mark.parametrize("I", SIZES)
def test_scored_lists_equal_the_oracle(ctx, I):
    bad = run_scoring(ctx, I, ["none", "excl", "cand"])
    assert not bad, bad


@gpu
@pytest.mark.parametrize("I", [63, 129])
def test_scored_lists_of_an_item_shard_equal_the_oracle(ctx, I):
    """item_offset > 0; the candidate rows hold items on either side of the shard, and k runs past what they allow."""
    bad = run_scoring(ctx, I, ["cand", "excl"], item_offset=70, extra=40)
    assert not bad, bad


def test_dense_reference_agrees_with_the_oracle_on_padding():
    """The NumPy reference's order and padding rule are the C oracle's (fp32, the one dense top-k the oracle has; it hands a
    -0.0 of its block back as it is, where the kernels read value + 0)."""
    I, n = 65, len(KINDS)
    preds = np.stack([content(kind, I) for kind in KINDS]).astype(np.float32)
    for mode in ("none", "excl", "cand"):
        kw = {} if mode == "none" else {mode: mask_rows(I, n)}
        for k in (1, 64, 193):
            ei, ev = dense_reference(preds, k, **kw)
            oi, ov = cref.topk_rows_f32(preds, 0, k, **kw)
            assert same_bits(ei, oi) and same_bits(ev, ov + np.float32(0)), (mode, k)


@gpu
@pytest.mark.parametrize("entry", ["el_dense_topk", "el_score_topk_f64"])
def test_half_given_mask_csr_is_refused_before_the_launch(ctx, entry):
    n, I, k = 4, 65, 10
    dtype = torch.float32 if entry == "el_dense_topk" else torch.float64
    indptr, indices = mask_rows(I, n)
    csr = ops.DeviceCSR(indptr, indices, I, ctx.device)
    ip, ix = ops._ptr(csr.indptr), ops._ptr(csr.indices)
    src = torch.ones((n, I), dtype=dtype, device=ctx.device)
    P, Q = torch.ones((n, 1), dtype=dtype, device=ctx.device), torch.ones((I, 1), dtype=dtype, device=ctx.device)
    for what, masks in (("cand CSR needs both arrays", (None, None, ip, None)),
                        ("cand CSR needs both arrays", (None, None, None, ix)),
                        ("excl_indptr without excl_indices", (ip, None, None, None))):
        out_idx = torch.full((n, k), -7, dtype=torch.int32, device=ctx.device)
        out_val = torch.full((n, k), -7.0, dtype=dtype, device=ctx.device)
        tail = (*masks, k, ops._ptr(out_idx), ops._ptr(out_val))
        if entry == "el_dense_topk":
            rc = ctx.lib.el_dense_topk(ctx.handle, ctx.stream(), ops._ptr(src), I, 0, n, I, *tail)
        else:
            rc = ctx.lib.el_score_topk_f64(ctx.handle, ctx.stream(), ops._ptr(P), ops._ptr(Q), None, 0, n, 0, I, 1, *tail)
        torch.cuda.synchronize()
        assert rc != 0
        assert (ctx.lib.el_last_error() or b"").decode() == f"{entry}: {what}"
        assert bool((out_idx == -7).all()) and bool((out_val == -7.0).all())


@gpu
@pytest.mark.parametrize("N", [1, 64, 65])
def test_rp3_row_cut_with_equal_keys_in_different_slices(ctx, N):
    """260 items are two column slices (192 + 68); items j and j + 192 have the same column of R, so the same S[i, j] and the
    same degree: equal keys meet in the merge of the slices' lists and rank by column."""
    from tests.helpers import rp3_ref
    from tests.helpers.rp3_ref import assert_w_equal, host_w, to_device
    rs = np.random.RandomState(5)
    U, I, dup = 150, 260, 192
    R = sp.random(U, I, density=0.15, random_state=rs, format="csc", dtype=np.float32)
    R.data[:] = rs.randint(1, 6, R.nnz).astype(np.float32)
    R = R.tolil()
    R[:, dup:] = R[:, :I - dup]
    R = sp.csr_matrix(R, dtype=np.float32)
    R.sort_indices()
    Piu, Pui, degree = rp3_ref.operands(R, 1.0, 0.4)
    W_ref = rp3_ref.build_w(Piu, Pui, degree, N, False)[0]
    dev = to_device(ops, ctx, Piu, Pui, degree)
    assert_w_equal(host_w(*ops.rp3_build(ctx, *dev, N, False)), W_ref)
