"""GPU: the VBPR kernels (el_vbpr.hip) at their edge shapes through the C ABI, against the float64 restatement tests/helpers/vbpr_ref.py.

U = 7, I = 65 (vbpr_ref.make_case), three foreign rows in front of every table.  F in {1, 3, 64, 100} x Fd in {1, 5, 20, 64} at
D = 65, B = 65 (every lane width and every elements-per-lane count of the segment kernels up to 4; F + Fd is odd, even, and a
multiple of 4); D in {1, 63, 64, 65, 2048} and B in {1, 2, 65, 4097} on two (F, Fd) pairs each; one shape with F + Fd + 1 > 256
(eight elements per lane).  What the batches plant is listed at vbpr_ref.make_case.

A lane group of the segment pass holds 8 sorted positions at these batch sizes and k_seg_combine adds at most 64 - 1 continuation
pieces (el_segcombine.h: fewer than `lpt` continuations, lpt <= 64), so a row with more than 8 x 64 = 512 occurrences takes
k_seg_combine_long whatever the row width: the "long_item" batch gives item 10 about 3400.

Tolerance of every compared array: 4 x the largest element-wise distance between the restatement's own float32 and float64 runs
on that case, floored at one float32 ulp of the array's largest magnitude (amf_ref.bound).  Every test prints kernel-to-float64
distance / bound per array before it asserts.  Integer results and the byte comparisons are exact.

Measured on an MI355X, kernel-to-float64 distance as a fraction of the bound, largest over the cases and the arrays compared:
gradients and loss 0.65 (gGi), variables after two / three steps with Adam 0.31, image scores and top-10 values 0.52.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import vbpr_ref
from tests.helpers.vbpr_ref import I, U

pytestmark = pytest.mark.gpu

PAD, FOREIGN = 3, 7.25
FS, FDS, DS, BS = [1, 3, 64, 100], [1, 5, 20, 64], [1, 63, 64, 65, 2048], [1, 2, 65, 4097]
SHAPES = sorted({(F, Fd, 65, 65) for F in FS for Fd in FDS}
                | {(F, Fd, D, 65) for (F, Fd) in ((3, 5), (64, 20)) for D in DS}
                | {(F, Fd, D, B) for (F, Fd, D) in ((3, 5, 65), (100, 20, 63)) for B in BS}
                | {(64, 20, 2048, 4097), (200, 64, 65, 65)})
shapes = pytest.mark.parametrize("F,Fd,D,B", SHAPES, ids=[f"F{F}-Fd{Fd}-D{D}-B{B}" for F, Fd, D, B in SHAPES])
GRADS = ("loss", "gBi", "gGu", "gGi", "gTu", "gE", "gBp")


@functools.lru_cache(maxsize=None)
def reference(F, Fd, D, B, kind="mixed", l_w=0.05, l_e=0.01, steps=False):
    """Everything the tests of one case compare with, from the restatement in float64 and float32 (computed once).  The first seed
    whose case keeps vbpr_ref's promise (no score at the clip bound) is the case."""
    for seed in range(16):
        try:
            return _reference(F, Fd, D, B, kind, l_w, l_e, steps, seed)
        except vbpr_ref.CaseRejected:
            continue
    raise AssertionError(f"no admissible case for F={F} Fd={Fd} D={D} B={B} {kind}")


def _reference(F, Fd, D, B, kind, l_w, l_e, steps, seed):
    case = vbpr_ref.make_case(F, Fd, D, B, kind, seed, l_w, l_e)
    b2 = vbpr_ref.make_case(F, Fd, D, B, "one_pair" if B > 1 else kind, seed + 100, l_w, l_e).batch      # leaves most items alone
    out, seen = {}, []
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = vbpr_ref.model_of(case, dt)
        seen.append(m)
        r = {"grads": [t.numpy() for t in m.gradients(case.batch)]}
        if steps:
            m.train_step(case.batch, case.lr)
            m.train_step(b2, case.lr)
            r["after2"] = [getattr(m, n).numpy().copy() for n in vbpr_ref.NAMES]
            m.train_step(case.batch, case.lr)
            r["after3"] = [getattr(m, n).numpy().copy() for n in vbpr_ref.NAMES]
        out[tag] = r
    vbpr_ref.check_case(seen)
    return case, b2, out


def compare(what, got, r64, r32, names=None):
    assert len(got) == len(r64)
    bad = []
    for k, (g, a, b) in enumerate(zip(got, r64, r32)):
        tol, dist = vbpr_ref.bound(a, b), vbpr_ref.distance(np.asarray(g).reshape(np.shape(a)), a)
        print(f"{what}[{names[k] if names else k}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((names[k] if names else k, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


class Raw:
    """The C ABI on tables that sit behind PAD foreign rows of one allocation each."""

    def __init__(self, ctx, case):
        self.ctx, self.case, dev = ctx, case, ctx.device
        self.F, self.Fd, self.D = case.F, case.Fd, case.D
        self.full = {}

        def table(name, shape, src=None):
            t = torch.full((shape[0] + PAD,) + tuple(shape[1:]), FOREIGN, dtype=torch.float32, device=dev)
            body = t[PAD:]
            body.zero_() if src is None else body.copy_(torch.from_numpy(np.ascontiguousarray(src)).reshape(body.shape))
            self.full[name] = t
            setattr(self, name, body)
            return body.data_ptr()

        N = self.Fd + 1
        mf = dict(Gu=table("Gu", (U, self.F), case.Gu), Gi=table("Gi", (I, self.F), case.Gi), Bi=table("Bi", (I,), case.Bi))
        for p in ("g", "m", "v"):
            mf.update({p + "Gu": table(p + "Gu", (U, self.F)), p + "Gi": table(p + "Gi", (I, self.F)), p + "Bi": table(p + "Bi", (I,))})
        st = dict(Tu=table("Tu", (U, self.Fd), case.Tu), EB=table("EB", (self.D, N), np.concatenate([case.E, case.Bp], axis=1)),
                  Feat=table("Feat", (I, self.D), case.feat))
        for p in ("g", "m", "v"):
            st.update({p + "Tu": table(p + "Tu", (U, self.Fd)), p + "EB": table(p + "EB", (self.D, N))})
        self.st = _lib.VbprState(mf=_lib.BprmfState(U=U, I=I, F=self.F, **mf), Fd=self.Fd, D=self.D, **st)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step, self.n_items = 0, None

    def grads(self, batch, hyper=None, rc_only=False, ws_short=0):
        case = hyper or self.case
        u, i, j = (torch.from_numpy(np.ascontiguousarray(b, dtype=np.int32)).to(self.ctx.device) for b in batch)
        B = int(u.numel())
        need = int(self.ctx.lib.el_vbpr_ws_bytes(self.ctx.handle, B, U, I, self.F, self.Fd, self.D))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=self.ctx.device)
        n = C.c_int64(-1)
        self.loss.zero_()
        rc = self.ctx.lib.el_vbpr_grads(self.ctx.handle, self.ctx.stream(), C.byref(self.st), C.c_void_p(u.data_ptr()),
                                        C.c_void_p(i.data_ptr()), C.c_void_p(j.data_ptr()), B, case.l_w, case.l_b, case.l_e,
                                        C.c_void_p(self.loss.data_ptr()), C.byref(n), C.c_void_p(ws.data_ptr()), need - ws_short)
        if not rc_only:
            _lib.check(rc, "el_vbpr_grads")
        torch.cuda.synchronize()
        self.n_items = int(n.value)
        return rc

    def apply(self, lr):
        self.step += 1
        _lib.check(self.ctx.lib.el_vbpr_apply(self.ctx.handle, self.ctx.stream(), C.byref(self.st), lr, self.step,
                                              float(ops.adam_lr_t(lr, self.step))), "el_vbpr_apply")
        torch.cuda.synchronize()

    def gradients(self):
        g = self.gEB.cpu().numpy()
        return [np.float64(self.loss.item()), self.gBi.cpu().numpy(), self.gGu.cpu().numpy(), self.gGi.cpu().numpy(),
                self.gTu.cpu().numpy(), g[:, :self.Fd], g[:, self.Fd:]]

    def variables(self):
        eb = self.EB.cpu().numpy()
        return [self.Bi.cpu().numpy(), self.Gu.cpu().numpy(), self.Gi.cpu().numpy(), self.Tu.cpu().numpy(), eb[:, :self.Fd], eb[:, self.Fd:]]

    def check_untouched(self, zero=()):
        """The foreign rows in front of every table are as they were; the named tables are all zero behind them."""
        for name, t in self.full.items():
            assert (t[:PAD] == FOREIGN).all(), f"{name}: foreign rows written"
        for name in zero:
            assert not getattr(self, name).any(), f"{name} not left zero"


def run_grads(ctx, key):
    case, _, ref = reference(*key)
    raw = Raw(ctx, case)
    raw.grads(case.batch)
    compare("grads", raw.gradients(), ref["f64"]["grads"], ref["f32"]["grads"], GRADS)
    u, i, j = case.batch
    items = np.union1d(i, j)
    assert raw.n_items == len(items)                                               # the products ran over the distinct items
    _, gBi, gGu, gGi, gTu, _, _ = raw.gradients()
    out_u, out_i = np.setdiff1d(np.arange(U), u), np.setdiff1d(np.arange(I), items)
    assert not gGu[out_u].any() and not gTu[out_u].any() and not gGi[out_i].any() and not gBi[out_i].any()
    raw.check_untouched(zero=("mGu", "vGu", "mGi", "vGi", "mBi", "vBi", "mTu", "vTu", "mEB", "vEB"))
    assert torch.equal(raw.Feat.cpu(), torch.from_numpy(case.feat))
    return raw, case


@shapes
def test_gradients_and_loss_against_the_fp64_restatement(ctx, F, Fd, D, B):
    raw, case = run_grads(ctx, (F, Fd, D, B))
    if B >= 16:                                                                    # the planted clipped triplet: no gradient through x
        x = vbpr_ref.model_of(case, torch.float64)
        x.gradients(case.batch)
        assert (x.xs[0] <= -81.0).sum() >= 1


@pytest.mark.parametrize("F,Fd", [(3, 5), (100, 20)])
@pytest.mark.parametrize("kind,B", [("one_user", 65), ("one_pair", 65), ("one_pair", 1), ("long_item", 4097), ("all_items", 4097),
                                    ("all_items", 65)])
def test_batch_shapes(ctx, F, Fd, kind, B):
    raw, case = run_grads(ctx, (F, Fd, 65, B, kind))
    u, i, j = case.batch
    if kind == "one_user":
        assert len(np.unique(u)) == 1
    if kind == "one_pair":
        assert raw.n_items == 2
    if kind == "long_item":
        assert (i == 10).sum() + (j == 10).sum() > 8 * 64 and (i == 10).any() and (j == 10).any()
    if kind == "all_items":
        assert raw.n_items == I                                                    # the products read the feature matrix in place


@pytest.mark.parametrize("l_w,l_e", [(0.0, 0.01), (0.05, 0.0), (0.0, 0.0)])
def test_regularisers_switched_off_apart_and_together(ctx, l_w, l_e):
    raw, case = run_grads(ctx, (3, 5, 65, 65, "mixed", l_w, l_e))
    if l_w == 0.0 and l_e == 0.0:
        _, _, ref = reference(3, 5, 65, 65)
        assert vbpr_ref.distance(raw.gradients()[5], ref["f64"]["grads"][5]) > 0    # l_e moved gE in the default case


@pytest.mark.parametrize("F,Fd,D,B", [(3, 5, 65, 65), (100, 20, 63, 4097), (64, 20, 2048, 4097)])
def test_two_runs_of_a_step_give_the_same_bytes(ctx, F, Fd, D, B):
    case, _, _ = reference(F, Fd, D, B)
    runs = []
    for _ in range(2):
        raw = Raw(ctx, case)
        raw.grads(case.batch)
        got = raw.gradients()[1:]
        raw.apply(case.lr)
        runs.append(got + raw.variables())
        raw.check_untouched(zero=("gGu", "gGi", "gBi", "gTu", "gEB"))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("F,Fd,D,B", [(3, 5, 65, 65), (100, 20, 63, 4097), (64, 64, 2048, 65)])
def test_three_steps_with_adam(ctx, F, Fd, D, B):
    case, b2, ref = reference(F, Fd, D, B, steps=True)
    raw = Raw(ctx, case)
    raw.grads(case.batch), raw.apply(case.lr)
    after1 = raw.variables()
    raw.grads(b2), raw.apply(case.lr)
    after2 = raw.variables()
    compare("two steps", after2, ref["f64"]["after2"], ref["f32"]["after2"], vbpr_ref.NAMES)
    # rows the second batch leaves alone got no gradient and still moved: Keras' Adam decays m, v and moves every row
    u1, items1 = np.unique(case.batch[0]), np.union1d(case.batch[1], case.batch[2])
    only1_u, only1_i = np.setdiff1d(u1, b2[0]), np.setdiff1d(items1, np.union1d(b2[1], b2[2]))
    assert len(only1_i) > 0
    for k, rows in ((0, only1_i), (1, only1_u), (2, only1_i), (3, only1_u)):
        if len(rows):
            assert (after2[k][rows] != after1[k][rows]).any(), vbpr_ref.NAMES[k]
    raw.grads(case.batch), raw.apply(case.lr)
    compare("three steps", raw.variables(), ref["f64"]["after3"], ref["f32"]["after3"], vbpr_ref.NAMES)
    raw.check_untouched(zero=("gGu", "gGi", "gBi", "gTu", "gEB"))


# ---- el_vbpr_item_image + el_score_topk / el_score_rank ------------------------------------------------------------------
K = 10


@functools.lru_cache(maxsize=None)
def scoring_case(F, Fd, D):
    """A case whose float64 scores keep, for EVERY user, adjacent scores down to rank K + 1 more than 100 x the bound apart (seeds are
    tried on the CPU until one does): the lists and positions are then decided by the function, not by rounding."""
    for seed in range(64):
        case = vbpr_ref.make_case(F, Fd, D, 65, seed=1000 + seed)
        case.Bi[5], case.Bi[6] = 0.1, -0.1                                          # (no planted clip here: ordinary biases)
        p64 = vbpr_ref.model_of(case, torch.float64).predict_all().numpy()
        p32 = vbpr_ref.model_of(case, torch.float32).predict_all().numpy()
        tol = vbpr_ref.bound(p64, p32)
        order = np.argsort(-p64, axis=1, kind="stable")
        top = np.take_along_axis(p64, order, axis=1)[:, :K + 2]
        if (np.abs(np.diff(top, axis=1)) > 100 * tol).all():
            return case, p64, p32, tol, order
    raise AssertionError("no seed separates the scores")


@pytest.mark.parametrize("F,Fd,D", [(1, 1, 1), (3, 5, 65), (64, 20, 2048), (100, 64, 63)])
def test_item_image_scores_lists_and_positions(ctx, F, Fd, D):
    case, p64, p32, tol, order = scoring_case(F, Fd, D)
    top = np.take_along_axis(p64, order, axis=1)[:, :K + 2]
    assert (np.abs(np.diff(top, axis=1)) > 100 * tol).all()                        # the precondition, for all users
    feat = torch.from_numpy(case.feat).to(ctx.device)
    st = ops.VbprDeviceState(ctx, case.Gu, case.Gi, case.Bi, case.Tu, case.E, case.Bp, feat)
    P, Q, bq = st.image()
    assert torch.equal(P[:, :F], st.base.Gu) and torch.equal(P[:, F:], st.Tu) and torch.equal(Q[:, :F], st.base.Gi)
    dense = (bq[None, :].double() + P.double() @ Q.double().T).cpu().numpy()       # the image's own scores, summed in float64
    dist = vbpr_ref.distance(dense, p64)
    print(f"image scores: |device - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
    assert dist <= tol
    idx, val = ops.score_topk(ctx, P, Q, bq, 0, U, K)
    vdist = vbpr_ref.distance(val.cpu().numpy(), np.take_along_axis(p64, order[:, :K], axis=1))
    print(f"top-{K} values: |device - f64| = {vdist:.3e}, bound {tol:.3e}, ratio {vdist / tol:.3f}")
    assert vdist <= tol
    assert np.array_equal(idx.cpu().numpy(), order[:, :K].astype(np.int32))        # every user, none left out
    # positions of the float64 rank-2 and rank-7 items of every user
    tgt = np.sort(order[:, [2, 7]], axis=1)
    targets = ops.DeviceCSR(np.arange(U + 1, dtype=np.int64) * 2, tgt.reshape(-1), I, ctx.device)
    pos = ops.score_rank(ctx, P, Q, bq, 0, U, targets).cpu().numpy().reshape(U, 2)
    want = np.array([[int(np.where(order[u] == t)[0][0]) for t in tgt[u]] for u in range(U)])
    assert np.array_equal(pos, want)


def test_refused_arguments_return_an_error_and_launch_nothing(ctx):
    case, _, _ = reference(3, 5, 65, 65)
    raw = Raw(ctx, case)
    lib, h, s = ctx.lib, ctx.handle, ctx.stream()

    def state(mf=None, **kw):
        st = _lib.VbprState.from_buffer_copy(raw.st)
        for k, v in kw.items():
            setattr(st, k, v)
        for k, v in (mf or {}).items():
            setattr(st.mf, k, v)
        return st

    before = [t.clone() for t in raw.full.values()]
    ctx.timing(True)
    try:
        ctx.timing_report()
        for k, st in enumerate([state(Tu=None), state(EB=None), state(Feat=None), state(gTu=None), state(gEB=None), state(Fd=0),
                                state(D=0), state(mf=dict(F=0)), state(mf=dict(F=507)), state(mf=dict(gGu=None)), state(mf=dict(Gi=None))]):
            good, raw.st = raw.st, st
            try:
                assert raw.grads(case.batch, rc_only=True) != 0, f"refused state {k} was accepted"
            finally:
                raw.st = good
        assert raw.grads(case.batch, rc_only=True, ws_short=257) != 0
        assert lib.el_vbpr_apply(h, s, C.byref(state(mTu=None)), 0.01, 1, 0.01) != 0
        assert lib.el_vbpr_item_image(h, s, C.byref(raw.st), None, None, None, None, 0) != 0
        assert lib.el_vbpr_ws_bytes(h, 0, U, I, 3, 5, 65) == 0 and lib.el_vbpr_ws_bytes(h, 65, U, I, 3, 0, 65) == 0
        assert ctx.timing_report() == {}
    finally:
        ctx.timing(False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, raw.full.values()))
