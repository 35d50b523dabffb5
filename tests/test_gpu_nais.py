"""GPU: the NAIS kernels (el_nais.hip) at their edge shapes through the C ABI, against the restatement tests/helpers/nais_ref.py (a
literal transcription of the reference's call / train_step / batch_predict for `concat`, gradients from autograd).

U = I = 600, L = 515, three foreign rows in front of every table.  Gradient cases draw Gi, Gj, W1, b1 on a 2^-4 grid so that no ReLU
falls on another side of zero in float32 than in float64 (nais_ref.check_exact).  With fism_piece = 8 histories and item lists take
one, a few and more than sixteen pieces; at B = 4097 the batch's pairs outgrow the scratch rows and the history pieces lengthen.
Every call has guard bytes behind its workspace and checks them.  Tolerance of every compared array: 4 x the distance between the
restatement's own float32 and float64 runs, floored at one float32 ulp of the array's largest magnitude; every test prints distance / bound before it asserts.

Measured on an MI355X, kernel-to-float64 distance as a fraction of the bound, largest over the cases and arrays compared: loss and ten
gradients 0.77 (gBu, whose bound is the one-ulp floor; gBi 0.65, gb1 0.60, the rest below 0.35), the FISM anchor 0.10, one Adam step
0.28 (W3), el_nais_scores 0.22, el_nais_forward 0.14.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import fism_ref, nais_ref
from tests.helpers.nais_ref import NAMES, bound, distance

pytestmark = pytest.mark.gpu

PAD, FOREIGN, K, GUARD = 3, 7.25, 10, 1 << 16
D = dict(F=10, B=65, Ws=32, alpha=0.5, beta=0.5, pad=True, loss="reference", piece=256)
CASES = [dict(D, F=F) for F in (1, 3, 10, 64, 100)] + [dict(D, Ws=w) for w in (1, 7)] + [dict(D, F=3, B=b) for b in (1, 2, 4097)] + \
        [dict(D, alpha=a) for a in (0.0, 1.0)] + [dict(D, beta=b) for b in (0.0, 1.0)] + [dict(D, pad=False), dict(D, loss="bce")] + \
        [dict(D, F=F, piece=8) for F in (3, 64)] + [dict(D, F=3, B=4097, piece=8)]
ident = lambda c: "-".join(f"{k}{v}" for k, v in c.items())                                 # noqa: E731
GRADS = ("loss",) + tuple("g" + n for n in NAMES)
SLOTS = NAMES + tuple("m" + n for n in NAMES) + tuple("v" + n for n in NAMES)


@functools.lru_cache(maxsize=None)
def reference(F, B, Ws, alpha, beta, pad, loss):
    case = nais_ref.make_case(F, B, Ws, alpha, beta)
    nais_ref.check_exact(case, case.batch)
    return case, [[np.asarray(t) for t in nais_ref.Model(case, dt, pad, loss).gradients(case.batch)] for dt in (torch.float64, torch.float32)]


def compare(what, got, r64, r32, names):
    bad = []
    for n, g, a, b in zip(names, got, r64, r32):
        tol, dist = bound(a, b), distance(np.asarray(g).reshape(np.shape(a)), a)
        print(f"{what}[{n}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((n, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


class Raw:
    """The C ABI on tables that sit behind PAD foreign rows of one allocation each."""

    def __init__(self, ctx, case, c, plant=None):
        self.ctx, self.case, dev = ctx, case, ctx.device
        self.full, ptr = {}, {}
        for n in NAMES:
            src = getattr(case, n)
            for pre in ("", "g", "m", "v"):
                t = torch.full((PAD + src.shape[0],) + src.shape[1:], FOREIGN, dtype=torch.float32, device=dev)
                t[PAD:].copy_(torch.from_numpy(src if pre == "" else (plant[pre + n] if plant and pre in "mv" else np.zeros_like(src))))
                self.full[pre + n], ptr[pre + n] = t, t[PAD:].data_ptr()
        self.index = [torch.from_numpy(a).to(dev) for a in ops.fism_history_index(case.indptr, case.indices, case.I)]
        self.coef = torch.from_numpy(case.coef).to(dev)
        self.slot = torch.full((case.U,), -1, dtype=torch.int32, device=dev)
        self.st = _lib.NaisState(U=case.U, I=case.I, nnz=int(case.indptr[-1]), F=case.F, Ws=case.Ws, alpha=case.alpha, beta_smooth=case.beta_smooth,
                                 l_b=case.l_b, loss_kind=ops.FISM_LOSSES[c["loss"]], pad_len=case.L if c["pad"] else 0,
                                 coef=self.coef.data_ptr(), h_indptr=self.index[0].data_ptr(), h_indices=self.index[1].data_ptr(),
                                 t_indptr=self.index[2].data_ptr(), t_indices=self.index[3].data_ptr(),
                                 slot=self.slot.data_ptr(), **ptr)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def call(self, batch, step=None, ws_short=0):
        dev, lib = self.ctx.device, self.ctx.lib
        u, i, y = (torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in batch)
        need = int(lib.el_nais_ws_bytes(self.ctx.handle, C.byref(self.st), len(u)))
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)                 # (GUARD bytes behind the workspace proper)
        head = (self.ctx.handle, self.ctx.stream(), C.byref(self.st), u.data_ptr(), i.data_ptr(), y.data_ptr(), len(u))
        tail = (self.loss.data_ptr(), ws.data_ptr(), need - ws_short)
        rc = lib.el_nais_grads(*head, *tail) if step is None else lib.el_nais_train_step(
            *head, step, float(ops.adam_lr_t(self.case.lr, step)), *tail)
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all(), "written behind el_nais_ws_bytes"
        return rc

    def arrays(self, names):
        return [self.full[n][PAD:].cpu().numpy() for n in names]

    def check_untouched(self):
        assert all((t[:PAD] == FOREIGN).all() for t in self.full.values()), "foreign rows written"
        assert (self.slot == -1).all(), "slot map not reset"


@pytest.mark.parametrize("c", CASES, ids=ident)
def test_loss_and_ten_gradients_against_the_restatement(ctx, c):
    case, (r64, r32) = reference(c["F"], c["B"], c["Ws"], c["alpha"], c["beta"], c["pad"], c["loss"])
    with ctx.option("fism_piece", c["piece"]):
        raw = Raw(ctx, case, c)
        assert raw.call(case.batch) == 0
    got = [np.float64(raw.loss.item())] + raw.arrays(GRADS[1:])
    compare("grads", got, r64, r32, GRADS)
    held = np.zeros(case.I, bool)
    for uu in set(case.batch[0].tolist()):
        held[case.hist[uu]] = True
    held[0] |= c["pad"]
    assert (~held).any() and not got[1][~held].any()                                       # gGi: items in no batch user's history
    raw.check_untouched()
    pairs, room = case.lens[case.batch[0]].sum(), max(c["B"], int(case.indptr[-1]) // c["piece"])
    if c["B"] == 4097 and c["piece"] == 8:
        assert pairs > 16 * 8 * room                                                       # (the history pieces grow to fit the scratch)
    elif c["piece"] == 8:
        for lens in (case.lens[np.unique(case.batch[0])], np.bincount(case.indices, minlength=case.I)):
            assert nais_ref.piece_counts(lens, 8) == (True, True, True)
        assert pairs <= 8 * room                                                           # (the history pieces stay 8 long)


@pytest.mark.parametrize("alpha,beta", [(0.5, 0.0), (0.25, 0.25)])
def test_uniform_attention_is_fism(ctx, alpha, beta):
    """W3 = 0, b3 = 0: FISM with exponent alpha + beta, regulariser beta = 1, lambda = gamma = l_b -- fism_ref in float64."""
    case = nais_ref.make_case(10, 65, 32, alpha, beta, uniform=True)
    fc = fism_ref.make_case(10, 65, alpha + beta)
    fc.Gi, fc.Gj, fc.beta, fc.lam, fc.gamma = case.Gi, case.Gj, 1.0, case.l_b, case.l_b
    r64, r32 = ([t.numpy() for t in fism_ref.Model(fc, dt).gradients(fc.batch)] for dt in (torch.float64, torch.float32))
    raw = Raw(ctx, case, D)
    assert raw.call(fc.batch) == 0
    compare("fism anchor", [np.float64(raw.loss.item())] + raw.arrays(GRADS[1:5]), r64, r32, GRADS[:5])


@pytest.mark.parametrize("step", [1, 3])
def test_one_train_step_with_adam(ctx, step):
    case, out, plant = nais_ref.make_case(10, 65), [], None
    if step == 3:
        rs = np.random.RandomState(5)
        plant = {p + n: (rs.uniform(-1e-3, 1e-3, getattr(case, n).shape) if p == "m" else rs.uniform(0, 1e-5, getattr(case, n).shape))
                 .astype(np.float32) for p in "mv" for n in NAMES}
    for dt in (torch.float64, torch.float32):
        m = nais_ref.Model(case, dt)
        if plant:
            m.m, m.v, m.step = {n: plant["m" + n].astype(m.m[n].dtype) for n in NAMES}, {n: plant["v" + n].astype(m.v[n].dtype) for n in NAMES}, 2
        m.train_step(case.batch, case.lr)
        out.append([getattr(m, n).numpy() for n in NAMES] + [m.m[n] for n in NAMES] + [m.v[n] for n in NAMES])
    raw = Raw(ctx, case, D, plant)
    assert raw.call(case.batch, step=step) == 0
    compare(f"step {step}", raw.arrays(SLOTS), out[0], out[1], SLOTS)
    assert all(not a.any() for a in raw.arrays(GRADS[1:]))
    raw.check_untouched()


@pytest.mark.parametrize("piece", [256, 8])
def test_two_runs_give_the_same_bytes(ctx, piece):
    case, runs = nais_ref.make_case(64, 65), []
    with ctx.option("fism_piece", piece):
        for _ in range(2):
            raw = Raw(ctx, case, D)
            assert raw.call(case.batch) == 0
            runs.append([raw.loss.cpu().numpy()] + raw.arrays(GRADS[1:]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("F", [3, 16, 100])
def test_scores_forward_and_topk_against_batch_predict(ctx, F, pad):
    case = nais_ref.make_case(F, 65, dyadic=False)
    want = sorted({int(np.argmin(np.abs(case.lens - n))) for n in (1, 2, 63, 64, 65, 255, 256, 257, 515)})
    users = want if F < 100 else want[:3]                                                  # (the CPU side of 2F = 200 stays at seconds)
    p64, p32 = (nais_ref.Model(case, dt, pad).batch_predict(users).numpy().astype(np.float64) for dt in (torch.float64, torch.float32))
    tol = bound(p64, p32)
    st = ops.NaisDeviceState(ctx, {n: getattr(case, n) for n in NAMES}, (case.indptr, case.indices), alpha=case.alpha, beta=case.beta_smooth,
                             l_b=case.l_b, padding="reference" if pad else "none")
    order = np.argsort(-p64, axis=1, kind="stable")
    top = np.take_along_axis(p64, order, axis=1)
    gaps = top[:, :K] - top[:, 1:K + 1]
    for r, u in enumerate(users):
        got = st.scores(u, u + 1).cpu().numpy()[0]
        uu = torch.full((case.I,), u, dtype=torch.int32, device=ctx.device)
        fwd = st.forward(uu, torch.arange(case.I, dtype=torch.int32, device=ctx.device)).cpu().numpy()
        ds, df = distance(got, p64[r]), distance(fwd, p64[r])
        print(f"user {u} (n = {case.lens[u]}): scores ratio {ds / tol:.3f}, forward ratio {df / tol:.3f}, bound {tol:.3e}")
        assert ds <= tol and df <= tol
        idx = st.recommend(u, u + 1, K)[0].cpu().numpy()[0]
        if gaps[r, K - 1] > 2 * tol:
            assert set(idx.tolist()) == set(order[r, :K].tolist())
        if (gaps[r] > 2 * tol).all():
            assert np.array_equal(idx, order[r, :K])
    assert (gaps[:, K - 1] > 2 * tol).any() and (st.slot == -1).all()


def test_the_workspace_holds_the_scan_over_many_more_samples_than_items(ctx):
    """B = 2^17 against I = 600: the scan over B + 1 piece counts needs more scratch than the one over I + 1 (Raw.call checks the guard)."""
    case = nais_ref.make_case(1, 1 << 17)
    raw = Raw(ctx, case, D)
    assert raw.call(case.batch) == 0 and np.isfinite(raw.loss.item())
    raw.check_untouched()


def test_a_short_workspace_is_refused_and_writes_nothing(ctx):
    case = nais_ref.make_case(3, 65)
    raw = Raw(ctx, case, D)
    before = [t.clone() for t in raw.full.values()]
    assert raw.call(case.batch, ws_short=1) != 0 and raw.call(case.batch, step=1, ws_short=1) != 0
    need = int(ctx.lib.el_nais_scores_ws_bytes(ctx.handle, C.byref(raw.st)))
    ws, out = torch.empty(need, dtype=torch.uint8, device=ctx.device), torch.full((case.I,), FOREIGN, device=ctx.device)
    assert ctx.lib.el_nais_scores(ctx.handle, ctx.stream(), C.byref(raw.st), 0, 1, out.data_ptr(), case.I, ws.data_ptr(), need - 1) != 0
    ids = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    assert ctx.lib.el_nais_forward(ctx.handle, ctx.stream(), C.byref(raw.st), ids.data_ptr(), ids.data_ptr(), 1, out.data_ptr(), ws.data_ptr(),
                                   need - 1) != 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, raw.full.values())) and (out == FOREIGN).all() and raw.loss.item() == 0
    raw.check_untouched()
