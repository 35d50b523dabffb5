"""GPU: the DMF kernels (el_dmf.hip) at their edge shapes, against the restatement tests/helpers/dmf_ref.py (a literal transcription of
the reference's call / train_step / get_recs, gradients from autograd).

U = I = 300; rating rows and columns of one, piece - 1, piece, piece + 1, 2 .. 5 and more than 16 pieces at fism_piece = 8; one user in
half of the samples; kernels that feed a ReLU on a 2^-4 grid (dmf_ref.check_exact), every y away from the clip edges (dmf_ref.check_clip).
Every step has guard bytes behind its workspace.  Tolerance of every compared array: 4 x the distance between the restatement's own
float32 and float64 runs, floored at one float32 ulp of the array's largest magnitude; every test prints distance / bound before it
asserts.

Measured on an MI355X, kernel-to-float64 distance as a fraction of the bound, largest over the cases and arrays compared: loss and
gradients 0.60 (guW0 of the row-cosine case with B = 1), three Adam steps 0.20 with train_step equal to grads + apply bit for bit, scores
0.30, `call` on pairs 0.29.  The case cosine/reference, towers (64, 32) / (5, 32), B = 513 has samples with a small y inside the clip,
which dy = -t / (y + 1e-7) weighs by 1 / y: the step keeps the last layer's outputs in double for them (k_dmf_last).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import dmf_ref
from tests.helpers.dmf_ref import bound, distance

pytestmark = pytest.mark.gpu

K, GUARD = 10, 1 << 16
COS, ROW, DOT = ("cosine", "reference"), ("cosine", "row"), ("dot", "reference")
CASES = [(COS, (64, 32), (5, 32), 513, 8), (COS, (32,), (256, 64, 32), 513, 256), (DOT, (5, 1), (1,), 513, 8), (ROW, (64, 32), (256, 32), 513, 8),
         (DOT, (64, 32), (64, 32), 1, 256), (DOT, (64, 32), (64, 5, 32), 513, 256), (ROW, (1, 32), (32,), 1, 8), (COS, (5, 1), (64, 1), 513, 8),
         (DOT, (256, 32), (64, 32), 513, 8)]
SEED = {(DOT, 1): 9, (ROW, 1): 7}          # B = 1: draws whose one y lies inside (0, 1) (the batch-axis cosine of ONE sample is an integer: no gradient)
ident = lambda c: "-".join(str(x).replace(" ", "") for x in (c if isinstance(c, tuple) else (c,)))                               # noqa: E731


@functools.lru_cache(maxsize=None)
def reference(sim, umlp, imlp, B):
    case = dmf_ref.make_case(umlp, imlp, B, seed=SEED.get((sim, B), 0))
    dmf_ref.check_exact(case, case.batch)
    r64, r32 = ([np.asarray(t) for t in dmf_ref.Model(case, *sim, dtype=dt).gradients(case.batch)] for dt in (torch.float64, torch.float32))
    dmf_ref.check_clip(r64[1], r32[1])
    assert B > 1 or (0 < r64[1][0] < 1 and all(g.any() for g in r64[2:])), "the one sample of a B = 1 case has no gradient"
    return case, r64, r32


def compare(what, got, r64, r32, names):
    bad = []
    for n, g, a, b in zip(names, got, r64, r32):
        tol, dist = bound(a, b), distance(np.asarray(g).reshape(np.shape(a)), a)
        print(f"{what}[{n}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((n, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


def device_state(ctx, case, sim, B=None):
    st = ops.DmfDeviceState(ctx, case.weights, case.csr, similarity=sim[0], cosine_axis=sim[1], max_rating=case.max_rating)
    if B:                                                                                    # GUARD bytes behind the step workspace proper
        st.need = int(ctx.lib.el_dmf_ws_bytes(ctx.handle, C.byref(st._c), B, _lib.EL_DMF_WS_STEP))
        st._ws0 = torch.full((st.need + GUARD,), 0xA5, dtype=torch.uint8, device=ctx.device)
    return st


def check_untouched(st):
    torch.cuda.synchronize()
    assert (st._ws0[st.need:] == 0xA5).all(), "written behind el_dmf_ws_bytes"
    assert (st.slot_u == -1).all() and (st.slot_i == -1).all(), "slot maps not reset"


def on_device(ctx, batch):
    return [torch.from_numpy(np.ascontiguousarray(b)).to(ctx.device) for b in batch]


@pytest.mark.parametrize("c", CASES, ids=ident)
def test_loss_and_every_gradient_against_the_restatement(ctx, c):
    sim, umlp, imlp, B, piece = c
    case, r64, r32 = reference(sim, umlp, imlp, B)
    names = dmf_ref.names(case)
    with ctx.option("fism_piece", piece):
        st = device_state(ctx, case, sim, B)
        st.grads(*on_device(ctx, case.batch))
        check_untouched(st)
    got = [np.float64(st.loss.item())] + [getattr(st, n[0] + "g" + n[1:]).cpu().numpy() for n in names]
    compare("grads", got, [r64[0]] + r64[2:], [r32[0]] + r32[2:], ["loss"] + ["g" + n for n in names])
    if B > 1:
        u, i = case.batch[0], case.batch[1]
        reached = (case.R[np.unique(u)] > 0).any(0)
        assert (u == 4).sum() >= (B - 9) // 2 and (~reached).any() and not got[1][~reached].any()   # rows of uW0 no batch row reaches
        if sim == DOT:
            assert (r64[1] < 0).any() and (r64[1] > 1).any()
        if piece == 8:
            for lens in ((case.R[np.unique(u)] > 0).sum(1), (case.R[:, np.unique(i)] > 0).sum(0), (case.R > 0).sum(0), (case.R > 0).sum(1)):
                assert {1, 7, 8, 9, 17, 28, 33} <= set(lens.tolist()) and (lens > 128).any()           # 1, 1, 1, 2, 3, 4, 5, > 16 pieces


@pytest.mark.parametrize("sim,piece", [(COS, 8), (ROW, 256), (DOT, 8)], ids=ident)
def test_three_adam_steps_fused_and_unfused(ctx, sim, piece):
    case = dmf_ref.make_case((64, 32), (5, 64, 32), 513)
    names, batches, out = dmf_ref.names(case), [case.batch, case.second, case.second], []
    once = (case.R[np.unique(case.batch[0])] > 0).any(0) & ~(case.R[np.unique(case.second[0])] > 0).any(0)
    assert once.any()                                                                        # rows of uW0 reached in step 1 only
    once = torch.from_numpy(once).to(ctx.device)
    for dt in (torch.float64, torch.float32):
        m = dmf_ref.Model(case, *sim, dtype=dt)
        losses = [m.train_step(b) for b in batches]
        out.append([np.float64(sum(losses))] + [x.numpy() for x in m.V] + m.m + m.v)
    with ctx.option("fism_piece", piece):
        fused, pair = device_state(ctx, case, sim, 513), device_state(ctx, case, sim, 513)
        for k, b in enumerate(batches):
            dev = on_device(ctx, b)
            before = fused.uW0.clone()
            fused.train_step(*dev, case.lr)
            pair.grads(*dev)
            pair.apply(case.lr)
            if k == 0:                                                                       # (a row whose users' samples are all clipped has g = 0)
                moving = once & (fused.umW0 != 0).any(1)
                assert moving.any()
            assert (before != fused.uW0)[moving].any(1).all()                                # g = 0 in steps 2 and 3: the rows keep moving
        check_untouched(fused), check_untouched(pair)
    slots = names + [n[0] + "m" + n[1:] for n in names] + [n[0] + "v" + n[1:] for n in names]
    for n in slots:
        assert torch.equal(getattr(fused, n), getattr(pair, n)), f"train_step != grads + apply at {n}"
    compare("three steps", [np.float64(fused.loss.item())] + [getattr(fused, n).cpu().numpy() for n in slots], out[0], out[1], ["loss"] + slots)


@pytest.mark.parametrize("sim", [COS, ROW, DOT], ids=ident)
def test_chunked_scores_and_top10_against_get_recs(ctx, sim):
    case = dmf_ref.make_case((64, 32), (64, 32), 1, last_bias=False)
    chunks = [(0, 128), (128, 256), (256, 300)]                                              # (the last chunk is shorter: another norm)
    p64, p32 = (torch.cat([dmf_ref.Model(case, *sim, dtype=dt).get_recs(s, e) for s, e in chunks]).numpy().astype(np.float64)
                for dt in (torch.float64, torch.float32))
    tol = bound(p64, p32)
    st = device_state(ctx, case, sim)
    got = torch.cat([st.scores(s, e) for s, e in chunks]).cpu().numpy()
    idx = torch.cat([st.recommend(s, e, K)[0] for s, e in chunks]).cpu().numpy()
    print(f"scores {ident(sim)}: |kernel - f64| = {distance(got, p64):.3e}, bound {tol:.3e}, ratio {distance(got, p64) / tol:.3f}")
    assert distance(got, p64) <= tol and len(st._qt) <= 2
    for qt in st._qt.values():                                                               # a stale Qt of a known chunk length is what gets used
        qt.zero_()
    assert sim == DOT or not st.scores(0, 128).any()
    order = np.argsort(-p64, axis=1, kind="stable")
    top = np.take_along_axis(p64, order, axis=1)
    gaps = top[:, :K] - top[:, 1:K + 1]
    sets, full = gaps[:, K - 1] > 2 * tol, (gaps > 2 * tol).all(1)
    assert sets.mean() >= 0.9                                                                # at most 10 % of the users are left out
    assert all(set(idx[r].tolist()) == set(order[r, :K].tolist()) for r in np.flatnonzero(sets))
    assert all(np.array_equal(idx[r], order[r, :K]) for r in np.flatnonzero(full))
    pu, pi = np.arange(65), (np.arange(65) * 3) % 300                                        # `call` on explicit pairs, one batch
    f64, f32 = (m.call(m.V, torch.as_tensor(pu), torch.as_tensor(pi)).numpy() for m in (dmf_ref.Model(case, *sim, dtype=dt)
                                                                                          for dt in (torch.float64, torch.float32)))
    fwd = st.forward(*on_device(ctx, (pu.astype(np.int32), pi.astype(np.int32)))).cpu().numpy()
    print(f"forward {ident(sim)}: ratio {distance(fwd, f64) / bound(f64, f32):.3f}")
    assert distance(fwd, f64) <= bound(f64, f32)


@pytest.mark.parametrize("umlp,imlp,word", [((8,) * 5, (8,), "layers"), ((257, 8), (8,), "width"), ((8, 4), (8, 5), "different widths")])
def test_refusals(ctx, umlp, imlp, word):
    rs = np.random.RandomState(0)
    w = {s: [(rs.rand(a, b).astype(np.float32), np.zeros(b, np.float32)) for a, b in zip((300,) + m[:-1], m)] for s, m in (("user", umlp), ("item", imlp))}
    case = dmf_ref.make_case((5, 32), (5, 32), 1)
    st = ops.DmfDeviceState(ctx, w, case.csr, max_rating=5.0)
    with pytest.raises(_lib.ElliotHipError, match=word):
        st.grads(*on_device(ctx, case.batch))
    with pytest.raises(_lib.ElliotHipError, match=word):
        st.towers()
