"""GPU: the FISM kernels (el_fism.hip) at their edge shapes through the C ABI, against the float64 restatement tests/helpers/fism_ref.py
(a literal transcription of the reference's call / train_step / batch_predict; what it plants is listed there).

U = I = 600, L = 515, three foreign rows in front of every table.  F in {1, 3, 10, 64, 100, 200} at B = 65 and B in {1, 2, 65, 4097} at
F in {3, 64}: every lane width and elements-per-lane count of the row split; alpha in {0, 0.5, 1}, pad_len in {0, L}, both loss
kinds.  At the default fism_piece = 256 the lists of 257 and 515 positions are cut in 2 and 3 pieces (the lane-group combine); with
fism_piece = 8 the lists of 255 .. 515 positions have 32 .. 65 pieces (the workgroup combine), those of 9 .. 34 positions 2 .. 5, so
the cut sum takes each of its three routes going forward and fanning out -- test_gradients asserts which lists do.

Tolerance of every compared array: amf_ref.bound -- 4 x the distance between the restatement's own float32 and float64 runs on that
case, floored at one float32 ulp of the array's largest magnitude.  Every test prints distance / bound before it asserts.

The top-10 comparison holds the item sets equal where the 10th/11th float64 gap exceeds twice the bound, and the order equal where
every gap down to the 11th does (two scores closer than the bound come out in either order in float32).

Measured on an MI355X, kernel-to-float64 distance as a fraction of the bound, largest over the cases and arrays compared:
gradients and loss 0.77 (gBu; the loss at most 0.17), variables and Adam slots after three steps 0.83 (mBu), top-10 values 0.61,
el_fism_forward 0.58.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import fism_ref
from tests.helpers.fism_ref import NAMES, U

pytestmark = pytest.mark.gpu

PAD, FOREIGN, K = 3, 7.25, 10
D = dict(alpha=0.5, pad=True, loss="reference", piece=256)
CASES = [dict(D, F=F, B=65) for F in (1, 3, 10, 64, 100, 200)] + [dict(D, F=F, B=B) for F in (3, 64) for B in (1, 2, 4097)] + \
        [dict(D, F=10, B=65, alpha=a) for a in (0.0, 1.0)] + [dict(D, F=10, B=65, pad=False), dict(D, F=10, B=65, loss="bce"),
                                                              dict(D, F=64, B=65, pad=False, loss="bce")] + \
        [dict(D, F=F, B=65, piece=8) for F in (3, 64)]
STEP_CASES = [dict(D, F=3, B=4097), dict(D, F=64, B=65, piece=8), dict(D, F=100, B=65, loss="bce"), dict(D, F=10, B=65, pad=False)]
ident = lambda c: "-".join(f"{k}{v}" for k, v in c.items())                                 # noqa: E731
cases = pytest.mark.parametrize("c", CASES, ids=ident)
step_cases = pytest.mark.parametrize("c", STEP_CASES, ids=ident)
GRADS = ("loss",) + tuple("g" + n for n in NAMES)


@functools.lru_cache(maxsize=None)
def reference(F, B, alpha, pad, loss, steps=False):
    """Everything the tests of one case compare with, from the restatement in float64 and float32 (computed once)."""
    case, out = fism_ref.make_case(F, B, alpha), {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = fism_ref.Model(case, dt, pad=pad, loss=loss)
        r = {"grads": [t.numpy() for t in m.gradients(case.batch)], "scores": m.batch_predict().numpy() if B == 65 else None}
        if steps:
            for b in (case.batch, case.second, case.batch):
                m.train_step(b, case.lr)
            r["after3"] = [getattr(m, n).numpy().copy() for n in NAMES] + [m.m[n].copy() for n in NAMES] + [m.v[n].copy() for n in NAMES]
        out[tag] = r
    return case, out


def ref_of(c, steps=False):
    return reference(c["F"], c["B"], c["alpha"], c["pad"], c["loss"], steps)


def compare(what, got, r64, r32, names):
    bad = []
    for n, g, a, b in zip(names, got, r64, r32):
        tol, dist = fism_ref.bound(a, b), fism_ref.distance(np.asarray(g).reshape(np.shape(a)), a)
        print(f"{what}[{n}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((n, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


class Raw:
    """The C ABI on tables that sit behind PAD foreign rows of one allocation each."""

    def __init__(self, ctx, case, c):
        self.ctx, self.case, dev = ctx, case, ctx.device
        self.full, ptr = {}, {}
        for n in NAMES:
            src = getattr(case, n)
            for pre in ("", "g", "m", "v"):
                t = torch.full((PAD + src.shape[0],) + src.shape[1:], FOREIGN, dtype=torch.float32, device=dev)
                t[PAD:].copy_(torch.from_numpy(src)) if pre == "" else t[PAD:].zero_()
                self.full[pre + n] = t
                setattr(self, pre + n, t[PAD:])
                ptr[pre + n] = t[PAD:].data_ptr()
        self.index = [torch.from_numpy(a).to(dev) for a in ops.fism_history_index(case.indptr, case.indices, case.I)]
        self.coef = torch.from_numpy(case.coef).to(dev)
        self.slot = torch.full((case.U,), -1, dtype=torch.int32, device=dev)
        self.nnz = int(case.indptr[-1])
        self.st = _lib.FismState(U=case.U, I=case.I, nnz=self.nnz, F=case.F, alpha=case.alpha, beta=case.beta, lambda_=case.lam,
                                 gamma=case.gamma, loss_kind=ops.FISM_LOSSES[c["loss"]], pad_len=case.L if c["pad"] else 0,
                                 coef=self.coef.data_ptr(), h_indptr=self.index[0].data_ptr(), h_indices=self.index[1].data_ptr(),
                                 t_indptr=self.index[2].data_ptr(), t_indices=self.index[3].data_ptr(), slot=self.slot.data_ptr(), **ptr)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def call(self, batch, step=None, ws_short=0, st=None):
        """el_fism_grads (step None) or el_fism_train_step; returns the status."""
        dev, lib = self.ctx.device, self.ctx.lib
        u, i, y = (torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in batch)
        need = int(lib.el_fism_ws_bytes(self.ctx.handle, len(u), self.case.U, self.case.I, self.nnz, self.case.F))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        head = (self.ctx.handle, self.ctx.stream(), C.byref(st or self.st), u.data_ptr(), i.data_ptr(), y.data_ptr(), len(u))
        tail = (self.loss.data_ptr(), ws.data_ptr(), need - ws_short)
        if step is None:
            rc = lib.el_fism_grads(*head, *tail)
        else:
            rc = lib.el_fism_train_step(*head, step, float(ops.adam_lr_t(self.case.lr, max(step, 1))), *tail)
        torch.cuda.synchronize()
        return rc

    def arrays(self, names):
        return [getattr(self, n).cpu().numpy() for n in names]

    def check_untouched(self, zero=()):
        assert all((t[:PAD] == FOREIGN).all() for t in self.full.values()), "foreign rows written"
        assert all(not getattr(self, n).any() for n in zero), "a table that must be zero is not"
        assert (self.slot == -1).all(), "slot map not reset"


def routes(lens, piece):
    """Which of the cut sum's routes lists of these lengths take: finished in place, lane-group combine, workgroup combine."""
    np_ = np.maximum(1, -(-np.asarray(lens) // piece))
    return {"place": bool((np_ == 1).any()), "group": bool(((np_ >= 2) & (np_ <= 16)).any()), "workgroup": bool((np_ > 16).any())}


@cases
def test_gradients_and_loss_against_the_fp64_restatement(ctx, c):
    case, ref = ref_of(c)
    with ctx.option("fism_piece", c["piece"]):
        raw = Raw(ctx, case, c)
        assert raw.call(case.batch) == 0
    got = [np.float64(raw.loss.item())] + raw.arrays(GRADS[1:])
    compare("grads", got, ref["f64"]["grads"], ref["f32"]["grads"], GRADS)
    u, i, _ = case.batch
    held = np.zeros(case.I, bool)
    for uu in set(u.tolist()):
        held[case.hist[uu]] = True
    if c["pad"]:
        held[0] = True
    idle_u, idle_i = np.setdiff1d(np.arange(U), u), np.setdiff1d(np.arange(case.I), i)
    assert (~held).any() and not got[1][~held].any()                                       # gGi: items in no batch user's history
    assert len(idle_i) and not got[2][idle_i].any() and not got[4][idle_i].any()           # gGj, gBi: never targeted
    assert len(idle_u) >= 300 and not got[3][idle_u].any()                                 # gBu: absent users
    raw.check_untouched(zero=tuple(p + n for p in "mv" for n in NAMES))
    item_lens = np.bincount(case.indices, minlength=case.I)
    if c["B"] >= 65:
        want = {"place": True, "group": True, "workgroup": c["piece"] == 8}
        assert routes(case.lens[np.unique(u)], c["piece"]) == want and routes(item_lens, c["piece"]) == want
        assert sorted(item_lens[[14, 13, 12, 11, 10]].tolist()) == [0, 1, 256, 257, 515] and not np.isin(np.unique(u), np.arange(340, 596)).any()
    if c["B"] == 4097:
        assert (i == 30).sum() > 700 and (u == 4).sum() > 2000


@step_cases
def test_three_steps_with_adam(ctx, c):
    case, ref = ref_of(c, steps=True)
    with ctx.option("fism_piece", c["piece"]):
        raw = Raw(ctx, case, c)
        for step, b in enumerate((case.batch, case.second, case.batch), 1):
            assert raw.call(b, step=step) == 0
    names = NAMES + tuple("m" + n for n in NAMES) + tuple("v" + n for n in NAMES)
    compare("three steps", raw.arrays(names), ref["f64"]["after3"], ref["f32"]["after3"], names)
    raw.check_untouched(zero=GRADS[1:])


@step_cases
def test_two_runs_give_the_same_bytes(ctx, c):
    case, _ = ref_of(c)
    runs = []
    with ctx.option("fism_piece", c["piece"]):
        for _ in range(2):
            raw = Raw(ctx, case, c)
            assert raw.call(case.batch) == 0
            runs.append([raw.loss.cpu().numpy()] + raw.arrays(GRADS[1:]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("F", [1, 10, 64, 200])
def test_user_image_topk_and_forward(ctx, F, pad):
    case, ref = reference(F, 65, 0.5, pad, "reference")
    p64, tol = ref["f64"]["scores"], fism_ref.bound(ref["f64"]["scores"], ref["f32"]["scores"])
    st = ops.FismDeviceState(ctx, case.Gi, case.Gj, case.Bu, case.Bi, (case.indptr, case.indices), alpha=case.alpha,
                             padding="reference" if pad else "none")
    assert st.pad_len == (case.L if pad else 0) and torch.equal(st.coef.cpu(), torch.from_numpy(case.coef))
    idx, val = st.recommend(st.image(), 0, U, K)
    order = np.argsort(-p64, axis=1, kind="stable")
    top = np.take_along_axis(p64, order, axis=1)
    vdist = fism_ref.distance(val.cpu().numpy(), top[:, :K])
    print(f"top-{K} values: |device - f64| = {vdist:.3e}, bound {tol:.3e}, ratio {vdist / tol:.3f}")
    assert vdist <= tol
    # the 10th/11th gap decides WHICH ten items a list holds; their order is decided where every gap down to the 11th is as wide
    # (two scores closer than the bound may come out in either order, or as one float, which tf.nn.top_k orders by index)
    gaps = top[:, :K] - top[:, 1:K + 1]
    decided, ordered = gaps[:, K - 1] > 2 * tol, (gaps > 2 * tol).all(1)
    got = idx.cpu().numpy()
    print(f"users decided: {decided.sum()} as sets, {ordered.sum()} in order, of {U}")
    assert decided.any() and np.array_equal(np.sort(got[decided], 1), np.sort(order[decided, :K], 1).astype(np.int32))
    assert ordered.any() and np.array_equal(got[ordered], order[ordered, :K].astype(np.int32))
    uu, ii = np.meshgrid(np.arange(U), np.arange(case.I), indexing="ij")
    pairs = [torch.from_numpy(x.reshape(-1).astype(np.int32)).to(ctx.device) for x in (uu, ii)]
    fdist = fism_ref.distance(st.forward(*pairs).cpu().numpy().reshape(p64.shape), p64)
    print(f"forward: |device - f64| = {fdist:.3e}, bound {tol:.3e}, ratio {fdist / tol:.3f}")
    assert fdist <= tol
    assert (st.slot == -1).all()


def test_refused_arguments_return_an_error_and_launch_nothing(ctx):
    c = CASES[1]
    case, _ = ref_of(c)
    raw = Raw(ctx, case, c)
    before = [t.clone() for t in raw.full.values()]

    def state(**kw):
        st = _lib.FismState.from_buffer_copy(raw.st)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    ctx.timing(True)
    try:
        ctx.timing_report()
        bad = [state(F=0), state(F=513), state(Gi=None), state(Bu=None), state(gGj=None), state(slot=None), state(coef=None),
               state(t_indptr=None), state(h_indices=None), state(loss_kind=2), state(pad_len=-1)]
        for k, st in enumerate(bad):
            assert raw.call(case.batch, st=st) != 0 and raw.call(case.batch, step=1, st=st) != 0, f"refused state {k} was accepted"
        assert raw.call(case.batch, ws_short=1) != 0 and raw.call(case.batch, step=1, ws_short=1) != 0
        assert raw.call(case.batch, step=0) != 0 and raw.call(case.batch, step=1, st=state(mBi=None)) != 0
        ws = ctx.lib.el_fism_ws_bytes
        assert ws(ctx.handle, 0, U, U, raw.nnz, 3) == 0 and ws(ctx.handle, 65, U, U, raw.nnz, 0) == 0
        assert ctx.lib.el_fism_user_image(ctx.handle, ctx.stream(), C.byref(raw.st), None, None, 0) != 0
        assert ctx.lib.el_fism_forward(ctx.handle, ctx.stream(), C.byref(state(F=513)), None, None, 4, None) != 0
        with ctx.option("fism_piece", 48):
            assert raw.call(case.batch) != 0 and ws(ctx.handle, 65, U, U, raw.nnz, 3) == 0
        assert ctx.timing_report() == {}
    finally:
        ctx.timing(False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, raw.full.values()))
    raw.check_untouched()


@pytest.mark.parametrize("r", [1, 4])
def test_ratio_sampler(ctx, r):
    import scipy.sparse as sp
    rs, n = np.random.RandomState(r), 65536
    m = sp.csr_matrix((rs.rand(50, 40) < 0.3).astype(np.float32))
    m.sort_indices()
    pos = ops.DeviceCSR(m.indptr, m.indices, 40, ctx.device)
    runs = [[t.cpu().numpy() for t in ops.pointwise_sample_ratio(ctx, pos, n, r, seed=11)] for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    u, i, y = runs[0]
    p, inside = 1.0 / (r + 1), m.toarray()[u, i] != 0
    print(f"neg_ratio {r}: positives {int(y.sum())} of {n}, expected {n * p:.0f} +- {np.sqrt(n * p * (1 - p)):.0f}")
    assert abs(y.sum() - n * p) <= 5 * np.sqrt(n * p * (1 - p))
    assert set(np.unique(y)) == {0.0, 1.0} and np.array_equal(inside, y == 1.0)
