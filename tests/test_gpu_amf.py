"""GPU: the AMF kernels (el_amf.hip) at their edge shapes against the float64 restatement tests/helpers/amf_ref.py.

Base shape U = 37, I = 23, three foreign rows in front of every table (so F = 1 and 7 take the scalar lanes from unaligned
pointers, F = 64 and 200 the 16-byte lanes); F in {1, 7, 64, 200}, B in {1, 63, 64, 65, 300, 2500}.  What every batch plants is
listed at amf_ref.make_case (B = 1 holds the first plant only).

Tolerance of every compared array: 4 x the largest element-wise distance between the restatement's own float32 and float64 runs
on that case, floored at one float32 ulp of the array's largest magnitude (amf_ref.bound; two float32 evaluations of one real
function may sit that far from the float64 value on opposite sides -- a factor 2 -- times the margin 2 of the AutoRec and
PureSVD tests).  Every test prints kernel-to-float64 distance / bound per array before it asserts.  Integer results and the
bit-equality checks are exact.

Measured on an MI355X, kernel-to-float64 distance as a fraction of the bound, largest over the 24 shapes and the arrays compared:
plain step 0.50, adversarial step 0.63, FGSM 0.41, MSAP 1 round 0.43, MSAP 3 rounds 0.67, second of two adversarial steps 1.00
(0.996 at F = 1, B = 1: gGu, 3.98e-8 of 3.99e-8; the next largest 0.87), three steps with Adam 0.29, l_w = 0.05 plain / adversarial
0.33 / 0.34 (DESIGN 3.27 has the table).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import amf_ref
from tests.helpers.amf_ref import PAD, I, U

pytestmark = pytest.mark.gpu

FS = [1, 7, 64, 200]
BS = [1, 63, 64, 65, 300, 2500]
FOREIGN = 7.25
SHAPES = [(F, B) for F in FS for B in BS]
shapes = pytest.mark.parametrize("F,B", SHAPES, ids=[f"F{F}-B{B}" for F, B in SHAPES])


def np32(t):
    return t.detach().to(torch.float32).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)


@functools.lru_cache(maxsize=None)
def reference(F, B, l_w=0.0):
    """Everything the tests of one shape compare with, from the restatement in float64 and float32 (computed once).  The first
    seed whose case keeps amf_ref's promise (no score at the clip bound, no row norm between 0 and 1e-3) is the shape's case."""
    for seed in range(16):
        try:
            return _reference(F, B, l_w, seed)
        except amf_ref.CaseRejected:
            continue
    raise AssertionError(f"no admissible case for F={F} B={B}")


def _reference(F, B, l_w, seed):
    case, case2 = amf_ref.make_case(F, B, seed), amf_ref.make_case(F, B, seed, second=True)
    case.l_w = l_w
    b1, b2 = case.batch, case2.batch
    seen = []

    def model(dtype, dGu=None, dGi=None):
        m = amf_ref.Model(case.Gu, case.Gi, case.Bi, case.l_w, case.l_b, case.eps, case.l_adv, dtype, dGu, dGi)
        seen.append(m)
        return m

    m = model(torch.float64)
    m.build_perturbation(b2)
    d0u, d0i = np32(m.dGu), np32(m.dGi)                        # a non-zero delta both sides start from (fp32 values)
    out = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        r = {}
        m = model(dt, d0u, d0i)
        r["plain"] = [t.numpy() for t in m.gradients(b1, False)]
        m = model(dt, d0u, d0i)
        r["adv"] = [t.numpy() for t in m.gradients(b1, True)] + [m.dGu.numpy(), m.dGi.numpy()]
        m = model(dt)
        m.build_perturbation(b1)
        r["fgsm"] = [m.dGu.numpy(), m.dGi.numpy()]
        for nb in (1, 3):
            m = model(dt)
            m.build_msap_perturbation(b1, 2.5 * case.eps / nb, nb)
            r[f"msap{nb}"] = [m.dGu.numpy(), m.dGi.numpy()]
        m = model(dt)
        m.gradients(b1, True)
        r["two"] = [t.numpy() for t in m.gradients(b2, True)] + [m.dGu.numpy(), m.dGi.numpy()]
        m = model(dt)
        for b in (b1, b2, b1):
            m.train_step(b, True, case.lr)
        r["train"] = [m.Bi.numpy(), m.Gu.numpy(), m.Gi.numpy()]
        out[tag] = r
    amf_ref.check_case(seen)
    return case, b2, (d0u, d0i), out


def compare(what, got, want):
    """got: arrays from the device; want: key into the reference bundle's (f64, f32) runs."""
    r64, r32 = want
    assert len(got) == len(r64)
    bad = []
    for k, (g, a, b) in enumerate(zip(got, r64, r32)):
        tol, dist = amf_ref.bound(a, b), amf_ref.distance(g, a)
        print(f"{what}[{k}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((k, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


class Raw:
    """The C ABI on tables that sit behind PAD foreign rows of one allocation each."""

    def __init__(self, ctx, case, delta=None):
        self.ctx, self.F, dev = ctx, case.F, ctx.device
        self.full = {}

        def table(name, rows, src=None, mat=True):
            t = torch.full((rows + PAD, self.F) if mat else (rows + PAD,), FOREIGN, dtype=torch.float32, device=dev)
            body = t[PAD:]
            body.zero_() if src is None else body.copy_(torch.from_numpy(np.ascontiguousarray(src)))
            self.full[name] = t
            setattr(self, name, body)
            return body.data_ptr()

        st = dict(Gu=table("Gu", U, case.Gu), Gi=table("Gi", I, case.Gi), Bi=table("Bi", I, case.Bi, mat=False))
        for p in ("g", "m", "v"):
            st.update({p + "Gu": table(p + "Gu", U), p + "Gi": table(p + "Gi", I), p + "Bi": table(p + "Bi", I, mat=False)})
        self.st = _lib.BprmfState(U=U, I=I, F=self.F, **st)
        du, di = delta if delta is not None else (None, None)
        self.rows_u = torch.zeros(U, dtype=torch.int32, device=dev)
        self.rows_i = torch.zeros(I, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=dev)
        self.d = _lib.AmfDelta(dGu=table("dGu", U, du), dGi=table("dGi", I, di), rows_u=self.rows_u.data_ptr(),
                               rows_i=self.rows_i.data_ptr(), counts=self.counts.data_ptr())
        if delta is not None:                                   # every row listed: a superset of the non-zero ones
            self.rows_u.copy_(torch.arange(U, dtype=torch.int32))
            self.rows_i.copy_(torch.arange(I, dtype=torch.int32))
            self.counts.copy_(torch.tensor([U, I], dtype=torch.int32))
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step = 0

    def _batch(self, batch):
        u, i, j = (torch.from_numpy(np.ascontiguousarray(b, dtype=np.int32)).to(self.ctx.device) for b in batch)
        B = int(u.numel())
        need = int(self.ctx.lib.el_amf_ws_bytes(B, U, I, self.F))
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device=self.ctx.device)
        return (u, i, j), (C.c_void_p(u.data_ptr()), C.c_void_p(i.data_ptr()), C.c_void_p(j.data_ptr()), B)

    def grads(self, case, batch, adversarial, rc_only=False):
        keep, head = self._batch(batch)
        self.loss.zero_()
        rc = self.ctx.lib.el_amf_grads(self.ctx.handle, self.ctx.stream(), C.byref(self.st), C.byref(self.d), *head, case.l_w, case.l_b,
                                       case.l_adv, case.eps, 1 if adversarial else 0, C.c_void_p(self.loss.data_ptr()),
                                       C.c_void_p(self.ws.data_ptr()), self.ws.numel())
        if not rc_only:
            _lib.check(rc, "el_amf_grads")
        torch.cuda.synchronize()
        del keep
        return rc

    def gradients(self):
        return [np.float64(self.loss.item()), self.gBi.cpu().numpy(), self.gGu.cpu().numpy(), self.gGi.cpu().numpy()]

    def delta(self):
        return [self.dGu.cpu().numpy(), self.dGi.cpu().numpy()]

    def apply(self, lr):
        self.step += 1
        _lib.check(self.ctx.lib.el_bprmf_apply(self.ctx.handle, self.ctx.stream(), C.byref(self.st), lr, _lib.EL_OPT_ADAM_TF_DENSE,
                                               self.step, float(ops.adam_lr_t(lr, self.step))), "el_bprmf_apply")

    def perturb(self, case, batch, nb_iter):
        keep, head = self._batch(batch)
        _lib.check(self.ctx.lib.el_amf_perturb(self.ctx.handle, self.ctx.stream(), C.byref(self.st), C.byref(self.d), *head, case.l_w,
                                               case.l_b, case.eps, 2.5 * case.eps / max(nb_iter, 1), nb_iter,
                                               C.c_void_p(self.ws.data_ptr()), self.ws.numel()), "el_amf_perturb")
        torch.cuda.synchronize()
        del keep

    def clear(self):
        _lib.check(self.ctx.lib.el_amf_delta_clear(self.ctx.handle, self.ctx.stream(), C.byref(self.st), C.byref(self.d)),
                   "el_amf_delta_clear")

    def check_untouched(self, zero=("gGu", "gGi", "gBi")):
        """The foreign rows in front of every table are as they were; the named tables are all zero behind them."""
        for name, t in self.full.items():
            assert (t[:PAD] == FOREIGN).all(), f"{name}: foreign rows written"
        for name in zero:
            assert not getattr(self, name).any(), f"{name} not left zero"

    def listed(self):
        nu, ni = self.counts.cpu().tolist()
        return set(self.rows_u[:nu].cpu().tolist()), set(self.rows_i[:ni].cpu().tolist()), nu, ni


@shapes
def test_plain_step_with_a_delta_in_place(ctx, F, B):
    case, _, d0, ref = reference(F, B)
    raw = Raw(ctx, case, d0)
    raw.grads(case, case.batch, False)
    compare("plain", raw.gradients(), (ref["f64"]["plain"], ref["f32"]["plain"]))
    assert np.array_equal(raw.delta()[0], d0[0]) and np.array_equal(raw.delta()[1], d0[1])       # a plain step leaves delta alone
    raw.check_untouched(zero=())


@shapes
def test_adversarial_step_gradients_loss_and_new_delta(ctx, F, B):
    case, _, d0, ref = reference(F, B)
    raw = Raw(ctx, case, d0)
    raw.grads(case, case.batch, True)
    compare("adversarial", raw.gradients() + raw.delta(), (ref["f64"]["adv"], ref["f32"]["adv"]))
    lu, li, nu, ni = raw.listed()
    u, i, j = case.batch
    assert lu == set(u.tolist()) and li == set(i.tolist()) | set(j.tolist()) and nu == len(lu) and ni == len(li)
    du, di = raw.delta()
    assert not du[sorted(set(range(U)) - lu)].any() and not di[sorted(set(range(I)) - li)].any()
    if B >= 8:
        assert not du[7].any()                                  # the user of the twin items: g is exactly 0, so is delta
    raw.check_untouched(zero=())


@shapes
@pytest.mark.parametrize("nb_iter", [0, 1, 3], ids=["fgsm", "msap1", "msap3"])
def test_stand_alone_perturbations(ctx, F, B, nb_iter):
    case, _, d0, ref = reference(F, B)
    raw = Raw(ctx, case, d0)                                    # an old delta is in place: the build starts from zero
    theta = [raw.Gu.clone(), raw.Gi.clone(), raw.Bi.clone()]
    raw.perturb(case, case.batch, nb_iter)
    key = "fgsm" if nb_iter == 0 else f"msap{nb_iter}"
    compare(key, raw.delta(), (ref["f64"][key], ref["f32"][key]))
    assert all(torch.equal(a, b) for a, b in zip(theta, (raw.Gu, raw.Gi, raw.Bi)))
    raw.check_untouched(zero=("gGu", "gGi", "gBi", "mGu", "mGi", "mBi", "vGu", "vGi", "vBi"))
    assert np.abs(np.concatenate([d.ravel() for d in raw.delta()])).max() <= case.eps * (1 + 1e-6)


@shapes
def test_two_consecutive_adversarial_steps(ctx, F, B):
    case, b2, _, ref = reference(F, B)
    raw = Raw(ctx, case)
    raw.grads(case, case.batch, True)
    raw.gGu.zero_(), raw.gGi.zero_(), raw.gBi.zero_()           # (what el_bprmf_apply would have done)
    raw.grads(case, b2, True)
    got = raw.gradients() + raw.delta()
    compare("second step", got, (ref["f64"]["two"], ref["f32"]["two"]))
    only1_u = sorted(set(case.batch[0].tolist()) - set(b2[0].tolist()))
    only1_i = sorted((set(case.batch[1].tolist()) | set(case.batch[2].tolist())) - (set(b2[1].tolist()) | set(b2[2].tolist())))
    assert not got[4][only1_u].any() and not got[5][only1_i].any()
    assert raw.listed()[0] == set(b2[0].tolist())
    # the same second step after delta was cleared in between must differ: the step read step 1's delta
    other = Raw(ctx, case)
    other.grads(case, case.batch, True)
    other.gGu.zero_(), other.gGi.zero_(), other.gBi.zero_()
    other.clear()
    assert not other.dGu.any() and not other.dGi.any() and other.listed()[2:] == (0, 0)
    other.grads(case, b2, True)
    cleared = other.gradients()
    assert not np.array_equal(cleared[2], got[2]) or not np.array_equal(cleared[3], got[3])
    assert np.array_equal(other.delta()[0], got[4]) and np.array_equal(other.delta()[1], got[5])     # FGSM reads the plain rows only


@shapes
def test_same_call_same_bytes(ctx, F, B):
    case, _, d0, _ = reference(F, B)
    runs = []
    for _ in range(2):
        raw = Raw(ctx, case, d0)
        raw.grads(case, case.batch, True)
        runs.append(raw.gradients()[1:] + raw.delta())
        raw.perturb(case, case.batch, 3)
        runs[-1] += raw.delta()
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("F,B", [(7, 65), (64, 300), (200, 2500)])
def test_three_adversarial_steps_with_adam(ctx, F, B):
    case, b2, _, ref = reference(F, B)
    raw = Raw(ctx, case)
    for b in (case.batch, b2, case.batch):
        raw.grads(case, b, True)
        raw.apply(case.lr)
    torch.cuda.synchronize()
    compare("three steps", [raw.Bi.cpu().numpy(), raw.Gu.cpu().numpy(), raw.Gi.cpu().numpy()], (ref["f64"]["train"], ref["f32"]["train"]))
    raw.check_untouched()


@pytest.mark.parametrize("F,B", [(7, 65), (200, 300)])
def test_weight_decay_reads_the_perturbed_rows(ctx, F, B):
    """l_w != 0 (the shapes above keep l_w = 0 for the exactly-zero row): the L2 term of a plain and an adversarial step."""
    case, _, d0, ref = reference(F, B, 0.05)
    for key, adv in (("plain", False), ("adv", True)):
        raw = Raw(ctx, case, d0)
        raw.grads(case, case.batch, adv)
        got = raw.gradients() + (raw.delta() if adv else [])
        compare(f"l_w {key}", got, (ref["f64"][key], ref["f32"][key]))


@pytest.mark.parametrize("F", FS)
def test_perturbed_tables_equal_the_fp32_host_sum(ctx, F):
    case, _, d0, _ = reference(F, 65)
    raw = Raw(ctx, case, d0)
    Pu = torch.full((U + PAD, F), FOREIGN, dtype=torch.float32, device=ctx.device)
    Pi = torch.full((I + PAD, F), FOREIGN, dtype=torch.float32, device=ctx.device)
    _lib.check(ctx.lib.el_amf_perturbed_tables(ctx.handle, ctx.stream(), C.byref(raw.st), C.byref(raw.d), C.c_void_p(Pu[PAD:].data_ptr()),
                                               C.c_void_p(Pi[PAD:].data_ptr())), "el_amf_perturbed_tables")
    assert (Pu[PAD:].cpu().numpy() == case.Gu + d0[0]).all() and (Pi[PAD:].cpu().numpy() == case.Gi + d0[1]).all()
    assert (Pu[:PAD] == FOREIGN).all() and (Pi[:PAD] == FOREIGN).all()


def test_device_state_scores_the_perturbed_tables(ctx):
    case, _, d0, _ = reference(64, 300)
    st = ops.AmfDeviceState(ctx, case.Gu, case.Gi, case.Bi)
    assert st.delta_is_zero and st.base.gGu is not None and not st.base.compact
    u, i, j = (torch.from_numpy(b).to(ctx.device) for b in case.batch)
    st.perturb(u, i, j, case.l_w, case.l_b, case.eps)
    assert not st.delta_is_zero
    Pu, Pi = st.perturbed_tables()
    assert torch.equal(Pu, st.base.Gu + st.dGu) and torch.equal(Pi, st.base.Gi + st.dGi)
    st.train_step(u, i, j, case.lr, case.l_w, case.l_b, case.l_adv, case.eps, True)
    st.train_step(u, i, j, case.lr, case.l_w, case.l_b, case.l_adv, case.eps, False)
    assert st.step == 2 and np.isfinite(st.pop_loss())
    st2 = ops.AmfDeviceState(ctx, case.Gu, case.Gi, case.Bi, st.dGu.cpu().numpy(), st.dGi.cpu().numpy())
    assert not st2.delta_is_zero and torch.equal(st2.dGu, st.dGu)
    st2.clear_delta()
    assert not st2.dGu.any() and not st2.dGi.any() and st2.delta_is_zero


def test_refused_arguments_return_an_error_and_launch_nothing(ctx):
    case, _, d0, _ = reference(7, 65)
    raw = Raw(ctx, case, d0)
    keep, head = raw._batch(case.batch)
    lib, h, s = ctx.lib, ctx.handle, ctx.stream()
    loss, ws, n = C.c_void_p(raw.loss.data_ptr()), C.c_void_p(raw.ws.data_ptr()), raw.ws.numel()
    tail = (0.0, 0.05, 0.7, 0.5, 1)

    def state(**kw):
        st = _lib.BprmfState.from_buffer_copy(raw.st)
        for k, v in kw.items():
            setattr(st, k, v)
        return C.byref(st)

    def delta(**kw):
        d = _lib.AmfDelta.from_buffer_copy(raw.d)
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    ok_st, ok_d = C.byref(raw.st), C.byref(raw.d)
    refused = [
        lambda: lib.el_amf_grads(h, s, None, ok_d, *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, None, *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, ok_d, None, *head[1:], *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, ok_d, *head[:3], 0, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, state(F=0), ok_d, *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, state(F=513), ok_d, *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, state(gGu=None), ok_d, *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, delta(dGi=None), *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, delta(counts=None), *head, *tail, loss, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, ok_d, *head, *tail, None, ws, n),
        lambda: lib.el_amf_grads(h, s, ok_st, ok_d, *head, *tail, loss, None, n),
        lambda: lib.el_amf_grads(h, s, ok_st, ok_d, *head, *tail, loss, ws, n - 1 - 256),
        lambda: lib.el_amf_grads(h, s, ok_st, ok_d, *head, 0.0, 0.05, 0.7, 0.5, 2, loss, ws, n),
        lambda: lib.el_amf_perturb(h, s, ok_st, ok_d, *head, 0.0, 0.05, 0.5, 0.1, -1, ws, n),
        lambda: lib.el_amf_perturb(h, s, ok_st, ok_d, *head, 0.0, 0.05, 0.5, 0.1, 2, ws, 16),
        lambda: lib.el_amf_perturb(h, s, state(Gi=None), ok_d, *head, 0.0, 0.05, 0.5, 0.1, 2, ws, n),
        lambda: lib.el_amf_delta_clear(h, s, ok_st, delta(rows_u=None)),
        lambda: lib.el_amf_perturbed_tables(h, s, ok_st, ok_d, None, ws),
    ]
    assert ctx.lib.el_amf_ws_bytes(0, U, I, 7) == 0 and ctx.lib.el_amf_ws_bytes(65, U, I, 0) == 0
    before = [t.clone() for t in raw.full.values()]
    ctx.timing(True)
    try:
        ctx.timing_report()
        for k, call in enumerate(refused):
            assert call() != 0, f"refused call {k} was accepted"
        assert ctx.timing_report() == {}
    finally:
        ctx.timing(False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, raw.full.values())) and raw.counts.cpu().tolist() == [U, I]
    del keep
