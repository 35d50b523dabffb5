"""GPU: the FM kernels (el_fm.hip) at their edge shapes through the C ABI, against the float64 restatement tests/helpers/fm_ref.py.

U = 7, I = 65 (300 for kind "every": one feature on every item, above the long-list threshold of k_fm_feat), three foreign rows in
front of every table.  F in {1, 3, 10, 64, 100, 200} at B = 65 and B in {1, 2, 65, 4097} at F in {3, 64}: every lane width and
elements-per-lane count of the row split, odd, even and multiple-of-4 widths; nF in {0, 1, 70}.  What the tables and batches plant
is listed at fm_ref.  At B = 4097 a lane group of the item pass holds 16 sorted positions and k_seg_combine adds fewer than 64
continuation pieces, so item 10 of kind "long_item" (about 800 samples) and user 2 (half of every batch) take k_seg_combine_long.

Tolerance of every compared array: amf_ref.bound -- 4 x the distance between the restatement's own float32 and float64 runs on that
case, floored at one float32 ulp of the array's largest magnitude.  Every test prints distance / bound before it asserts.

Measured on an MI355X, kernel-to-float64 distance as a fraction of the bound, largest over the cases and arrays compared:
gradients and loss 0.63 (gw), top-10 values 0.19, el_fm_forward 0.32, variables and Adam slots after three steps 0.35 (vE; the
global bias and its two slots, which the state keeps as doubles, at most 0.19).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import fm_ref
from tests.helpers.fm_ref import NAMES, U

pytestmark = pytest.mark.gpu

PAD, FOREIGN, K = 3, 7.25, 10
CASES = sorted({(F, 65, 70, "mixed") for F in (1, 3, 10, 64, 100, 200)} | {(F, B, 70, "mixed") for F in (3, 64) for B in (1, 2, 65, 4097)}
               | {(F, 4097, 70, "long_item") for F in (3, 64)} | {(F, 65, 70, "every") for F in (3, 64, 100)}
               | {(10, 65, 1, "mixed"), (10, 65, 0, "mixed"), (64, 4097, 0, "mixed")})
cases = pytest.mark.parametrize("F,B,nF,kind", CASES, ids=[f"F{F}-B{B}-nF{nF}-{kind}" for F, B, nF, kind in CASES])
STEP_CASES = [(3, 65, 70, "mixed"), (64, 4097, 70, "long_item"), (100, 65, 70, "every"), (10, 65, 0, "mixed")]


@functools.lru_cache(maxsize=None)
def reference(F, B, nF, kind, steps=False):
    """Everything the tests of one case compare with, from the restatement in float64 and float32 (computed once)."""
    case, out = fm_ref.make_case(F, B, nF, kind), {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = fm_ref.Model(case, dt)
        r = {"grads": [t.numpy() for t in m.gradients(case.batch)], "scores": m.predict_all().numpy()}
        if steps:
            for b in (case.batch, case.second, case.batch):
                m.train_step(b, case.lr)
            r["after3"] = [getattr(m, n).numpy().copy() for n in NAMES] + [m.m[n].numpy().copy() for n in NAMES] + \
                          [m.v[n].numpy().copy() for n in NAMES]
        out[tag] = r
    return case, out


def compare(what, got, r64, r32, names):
    bad = []
    for n, g, a, b in zip(names, got, r64, r32):
        tol, dist = fm_ref.bound(a, b), fm_ref.distance(np.asarray(g).reshape(np.shape(a)), a)
        print(f"{what}[{n}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((n, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


class Raw:
    """The C ABI on tables that sit behind PAD foreign rows of one allocation each."""

    def __init__(self, ctx, case):
        self.ctx, self.case, dev = ctx, case, ctx.device
        self.N, self.full = case.U + case.I + case.nF, {}
        ptr = {}
        for n, src in (("E", case.E), ("w", case.w), ("g0", np.array([case.g0]))):
            for pre in ("", "g", "m", "v"):
                dt = torch.float64 if pre + n in ("gg0", "mg0", "vg0") else torch.float32   # (el_fm_state: the global bias's doubles)
                t = torch.full((PAD + src.shape[0],) + src.shape[1:], FOREIGN, dtype=dt, device=dev)
                t[PAD:].copy_(torch.from_numpy(src)) if pre == "" else t[PAD:].zero_()
                self.full[pre + n] = t
                setattr(self, pre + n, t[PAD:])
                ptr[pre + n] = t[PAD:].data_ptr()
        self.full["g0d"] = torch.tensor([FOREIGN] * PAD + [float(case.g0)], dtype=torch.float64, device=dev)
        ptr["g0d"] = self.full["g0d"][PAD:].data_ptr()
        self.index = [torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev) for a in ops.fm_attribute_index(case.feats, case.nF)]
        longest = int(np.diff(self.index[2].cpu().numpy()).max()) if case.nF else 0
        self.slot = torch.full((case.I,), -1, dtype=torch.int32, device=dev)
        self.st = _lib.FmState(U=case.U, I=case.I, nF=case.nF, F=case.F, a_indptr=self.index[0].data_ptr(), a_indices=self.index[1].data_ptr(),
                               t_indptr=self.index[2].data_ptr(), t_indices=self.index[3].data_ptr(), t_longest=longest,
                               slot=self.slot.data_ptr(), **ptr)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step = 0

    def call(self, batch, step=None, ws_short=0, st=None):
        """el_fm_grads (step None) or el_fm_train_step; returns the status."""
        dev, lib = self.ctx.device, self.ctx.lib
        u, i, y = (torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in batch)
        need = int(lib.el_fm_ws_bytes(self.ctx.handle, len(u), self.case.U, self.case.I, self.case.F))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        head = (self.ctx.handle, self.ctx.stream(), C.byref(st or self.st), u.data_ptr(), i.data_ptr(), y.data_ptr(), len(u))
        tail = (self.loss.data_ptr(), ws.data_ptr(), need - ws_short)
        if step is None:
            rc = lib.el_fm_grads(*head, *tail)
        else:
            rc = lib.el_fm_train_step(*head, step, float(ops.adam_lr_t(self.case.lr, max(step, 1))), *tail)
        torch.cuda.synchronize()
        return rc

    def arrays(self, names):
        return [getattr(self, n).cpu().numpy() for n in names]

    def check_untouched(self, zero=()):
        assert all((t[:PAD] == FOREIGN).all() for t in self.full.values()), "foreign rows written"
        assert all(not getattr(self, n).any() for n in zero), "a table that must be zero is not"
        assert (self.slot == -1).all(), "slot map not reset"


@cases
def test_gradients_and_loss_against_the_fp64_restatement(ctx, F, B, nF, kind):
    case, ref = reference(F, B, nF, kind)
    raw = Raw(ctx, case)
    assert raw.call(case.batch) == 0
    got = [np.float64(raw.loss.item())] + raw.arrays(("gE", "gw", "gg0"))
    compare("grads", got, ref["f64"]["grads"], ref["f32"]["grads"], ("loss", "gE", "gw", "gg0"))
    u, i, _ = case.batch
    active = set(u.tolist()) | {U + x for x in i.tolist()} | {U + case.I + f for x in set(i.tolist()) for f in case.feats[x]}
    idle = np.setdiff1d(np.arange(raw.N), sorted(active))
    assert len(idle) > 0 and not got[1][idle].any() and not got[2][idle].any()     # rows of no active index: exactly zero
    raw.check_untouched(zero=("mE", "vE", "mw", "vw", "mg0", "vg0"))
    if kind == "long_item":
        assert (i == 10).sum() > 8 * 64
    if kind == "every":
        assert case.I > 256 and all(67 in f for f in case.feats)


@pytest.mark.parametrize("F,B,nF,kind", STEP_CASES)
def test_three_steps_with_adam(ctx, F, B, nF, kind):
    case, ref = reference(F, B, nF, kind, steps=True)
    raw = Raw(ctx, case)
    for step, b in enumerate((case.batch, case.second, case.batch), 1):
        assert raw.call(b, step=step) == 0
    names = NAMES + tuple("m" + n for n in NAMES) + tuple("v" + n for n in NAMES)
    compare("three steps", raw.arrays(names), ref["f64"]["after3"], ref["f32"]["after3"], names)
    raw.check_untouched(zero=("gE", "gw", "gg0"))


@pytest.mark.parametrize("F,B,nF,kind", STEP_CASES)
def test_two_runs_give_the_same_bytes(ctx, F, B, nF, kind):
    case, _ = reference(F, B, nF, kind)
    runs = []
    for _ in range(2):
        raw = Raw(ctx, case)
        assert raw.call(case.batch) == 0
        runs.append([raw.loss.cpu().numpy()] + raw.arrays(("gE", "gw", "gg0")))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


@pytest.mark.parametrize("F,nF,kind", [(1, 70, "mixed"), (10, 70, "mixed"), (64, 70, "every"), (200, 1, "mixed"), (10, 0, "mixed")])
def test_item_image_topk_and_forward(ctx, F, nF, kind):
    case, ref = reference(F, 65, nF, kind)
    p64, tol = ref["f64"]["scores"], fm_ref.bound(ref["f64"]["scores"], ref["f32"]["scores"])
    st = ops.FmDeviceState(ctx, case.U, case.I, case.E, case.w, case.g0, item_features=case.feats, n_features=nF)
    Q, bq = st.image()
    idx, val = st.recommend(Q, bq, 0, U, K)
    order = np.argsort(-p64, axis=1, kind="stable")
    top = np.take_along_axis(p64, order, axis=1)
    vdist = fm_ref.distance(val.cpu().numpy(), top[:, :K])
    print(f"top-{K} values: |device - f64| = {vdist:.3e}, bound {tol:.3e}, ratio {vdist / tol:.3f}")
    assert vdist <= tol
    decided = (top[:, K - 1] - top[:, K]) > 2 * tol
    assert decided.any() and np.array_equal(idx.cpu().numpy()[decided], order[decided, :K].astype(np.int32))
    uu, ii = np.meshgrid(np.arange(U), np.arange(case.I), indexing="ij")
    pairs = [torch.from_numpy(x.reshape(-1).astype(np.int32)).to(ctx.device) for x in (uu, ii)]
    fdist = fm_ref.distance(st.forward(*pairs).cpu().numpy().reshape(p64.shape), p64)
    print(f"forward: |device - f64| = {fdist:.3e}, bound {tol:.3e}, ratio {fdist / tol:.3f}")
    assert fdist <= tol
    assert (st.slot == -1).all()


def test_labels_are_the_ratings_of_positives_and_zero_for_negatives(ctx):
    import scipy.sparse as sp
    rs = np.random.RandomState(3)
    dense = np.where(rs.rand(U, 65) < 0.3, rs.randint(1, 6, (U, 65)), 0).astype(np.float32)
    dense[0, 0] = dense[0, 64] = 4.0                                               # the first and the last column of a row
    m = sp.csr_matrix(dense)
    for r in range(U):                                                             # the columns of every row descending
        s, e = m.indptr[r], m.indptr[r + 1]
        m.indices[s:e], m.data[s:e] = m.indices[s:e][::-1].copy(), m.data[s:e][::-1].copy()
    ratings = ops.fm_ratings_csr(ctx, sp.csr_matrix((m.data, m.indices, m.indptr), shape=m.shape))
    uu, ii = np.meshgrid(np.arange(U), np.arange(65), indexing="ij")
    u, i = (torch.from_numpy(x.reshape(-1).astype(np.int32)).to(ctx.device) for x in (uu, ii))
    flips = (rs.rand(U * 65) < 0.5).astype(np.float32)
    flips[0], flips[64] = 1.0, 1.0                                                 # (0, 0) and (0, 64) are asked for as positives
    coin = torch.from_numpy(flips).to(ctx.device)
    y = ops.fm_labels(ctx, ratings, u, i, coin).cpu().numpy().reshape(U, 65)
    want = dense * coin.cpu().numpy().reshape(U, 65)
    assert np.array_equal(y, want) and (want[:, 0] > 0).any() and (want[:, 64] > 0).any()


def test_refused_arguments_return_an_error_and_launch_nothing(ctx):
    case, _ = reference(3, 65, 70, "mixed")
    raw = Raw(ctx, case)
    before = [t.clone() for t in raw.full.values()]

    def state(**kw):
        st = _lib.FmState.from_buffer_copy(raw.st)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    ctx.timing(True)
    try:
        ctx.timing_report()
        for k, st in enumerate([state(F=0), state(F=513), state(nF=-1), state(E=None), state(gE=None), state(slot=None), state(t_indptr=None)]):
            assert raw.call(case.batch, st=st) != 0 and raw.call(case.batch, step=1, st=st) != 0, f"refused state {k} was accepted"
        assert raw.call(case.batch, ws_short=1) != 0 and raw.call(case.batch, step=1, ws_short=1) != 0
        assert raw.call(case.batch, step=0) != 0 and raw.call(case.batch, step=1, st=state(mw=None)) != 0
        assert ctx.lib.el_fm_ws_bytes(ctx.handle, 0, U, 65, 3) == 0 and ctx.lib.el_fm_ws_bytes(ctx.handle, 65, U, 65, 0) == 0
        assert ctx.lib.el_fm_item_image(ctx.handle, ctx.stream(), C.byref(raw.st), None, None) != 0
        assert ctx.timing_report() == {}
    finally:
        ctx.timing(False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, raw.full.values()))
    raw.check_untouched()
