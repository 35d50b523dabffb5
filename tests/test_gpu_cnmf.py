"""GPU: the ConvNeuMF kernels (el_cnmf.hip) at their edge shapes, against the restatement tests/helpers/cnmf_ref.py (conv2d on the
explicit outer product, gradients from autograd).

U = 70, I = 45.  Cases (F, channels, kernels = strides, B): the default tower's family with B one past a block; a dropped last row and
column with channel counts far from a tile; L = 1; a pyramid down to 1 x 1; mixed kernels with K = 4 * 33, 33 and 64 channels (W_2 past
its LDS stage); 7 -> 3 -> 1 with C_L = 1; the default F = 100 (625 layer-2 pixels = 19 row tiles + 17 rows).  Every conv pre-activation
is exact in float32 (cnmf_ref.check_exact), no x_ui - x_uj lies near the clip.  Every step has guard bytes behind its workspace.
Tolerance of every compared array: 4 x the distance between the restatement's own float32 and float64 runs, floored at one float32 ulp
of the array's largest magnitude; every test prints distance / bound before it asserts.

Measured on an MI355X, the largest distance / bound over the cases and arrays compared: loss and gradients 0.25 (gD2), three Adam steps
0.50 (mW0) with train_step equal to grads + apply bit for bit, chunked scores 0.07, `call` on pairs 0.07.
"""
import functools

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.helpers import cnmf_ref
from tests.helpers.cnmf_ref import bound, distance

pytestmark = pytest.mark.gpu

K, GUARD = 10, 1 << 16
CASES = [(8, (1, 32, 32), (2, 2), 513), (9, (1, 5, 3), (2, 2), 513), (12, (1, 4), (3,), 1), (16, (1, 8, 8, 8, 8), (2, 2, 2, 2), 65),
         (18, (1, 33, 64), (3, 2), 513), (7, (1, 64, 1), (2, 3), 2), (100, (1, 32, 32), (2, 2), 3)]
GRID = {16: dict(ebits=1, wbits=1)}                                         # four layers deep: a coarser grid keeps every sum exact
SCORE_SEED = {8: 0, 18: 0}
ident = lambda c: "-".join(str(x).replace(" ", "") for x in (c if isinstance(c, tuple) else (c,)))       # noqa: E731


@functools.lru_cache(maxsize=None)
def reference(F, channels, kernels, B, seed=0):
    case = cnmf_ref.make_case(F, channels, kernels, B, seed=seed, **GRID.get(F, {}))
    cnmf_ref.check_exact(case, case.batch)
    r64, r32 = ([np.asarray(t) for t in cnmf_ref.Model(case, dt).gradients(case.batch)] for dt in (torch.float64, torch.float32))
    assert B < 3 or ((r64[1] < 0).any() and (r64[1] > 0).any())
    return case, r64, r32


def compare(what, got, r64, r32, names):
    bad = []
    for n, g, a, b in zip(names, got, r64, r32):
        tol, dist = bound(a, b), distance(np.asarray(g).reshape(np.shape(a)), a)
        print(f"{what}[{n}]: |kernel - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((n, dist, tol))
    assert not bad, f"{what}: outside 4 x |f32 - f64| of the restatement: {bad}"


def device_state(ctx, case, B=None, dropout=0.0):
    st = ops.ConvNeuMfDeviceState(ctx, case.weights, case.channels, case.kernels, case.kernels, l_w=case.l_w, dropout=dropout)
    if B:                                                                                    # GUARD bytes behind the step workspace proper
        st.need = st.ws_bytes(B, _lib.EL_CNMF_WS_STEP)
        st._ws0 = torch.full((st.need + GUARD,), 0xA5, dtype=torch.uint8, device=ctx.device)
    return st


def check_untouched(st):
    torch.cuda.synchronize()
    assert (st._ws0[st.need:] == 0xA5).all(), "written behind el_cnmf_ws_bytes"


def on_device(ctx, batch):
    return [torch.from_numpy(np.ascontiguousarray(b)).to(ctx.device) for b in batch]


@pytest.mark.parametrize("c", CASES, ids=ident)
def test_loss_and_every_gradient_against_the_restatement(ctx, c):
    F, channels, kernels, B = c
    case, r64, r32 = reference(*c)
    names = cnmf_ref.names(case)
    st = device_state(ctx, case, B)
    runs = []
    for _ in range(2):
        st.loss.zero_()
        st.grads(*on_device(ctx, case.batch))
        check_untouched(st)
        runs.append([np.float64(st.loss.item())] + [getattr(st, "g" + n).cpu().numpy() for n in names])
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs differ"
    compare("grads", runs[0], [r64[0]] + r64[2:], [r32[0]] + r32[2:], ["loss"] + ["g" + n for n in names])
    if F == 9:                                               # row and column 8 of the map reach no conv gradient: the regulariser's alone
        u, cnt = np.unique(case.batch[0], return_counts=True)
        reg = np.float64(np.float32(case.l_w)) * cnt[:, None] * case.weights["P"][u].astype(np.float64)   # l_w p per occurrence, exact in double
        assert (r64[2][u, :8] != reg[:, :8]).any() and reg[:, 8].any()
        assert np.array_equal(runs[0][1][u, 8], reg[:, 8].astype(np.float32))


@pytest.mark.parametrize("c,dropout", [(CASES[1], 0.5), (CASES[4], 0.0)], ids=ident)
def test_three_adam_steps_fused_and_unfused(ctx, c, dropout):
    F, channels, kernels, B = c
    case = reference(*c)[0]
    names, batches, out = cnmf_ref.names(case), [case.batch, case.second, case.second], []
    once = np.setdiff1d(case.batch[0], case.second[0])
    assert once.size                                                                         # rows of P met in step 1 only
    fused, pair = device_state(ctx, case, B, dropout), device_state(ctx, case, B, dropout)
    masks = [fused.dropout_masks(k + 1, B).cpu().numpy() if dropout else None for k in range(3)]
    assert not dropout or (all(set(np.unique(m)) == {0.0, 2.0} for m in masks) and not np.array_equal(masks[0][0], masks[0][1])
                           and not np.array_equal(masks[0], masks[1]))
    for dt in (torch.float64, torch.float32):
        m = cnmf_ref.Model(case, dt)
        losses = [m.train_step(b, mk) for b, mk in zip(batches, masks)]
        out.append([np.float64(sum(losses))] + [x.numpy() for x in m.V] + m.m + m.v)
    for k, b in enumerate(batches):
        dev = on_device(ctx, b)
        before = fused.P.clone()
        fused.train_step(*dev, case.lr)
        pair.grads(*dev)
        pair.apply(case.lr)
        assert (before != fused.P)[torch.from_numpy(once).long().to(ctx.device)].any(1).all()    # g = 0 in steps 2 and 3: the rows keep moving
    check_untouched(fused), check_untouched(pair)
    slots = names + ["m" + n for n in names] + ["v" + n for n in names]
    for n in slots:
        assert torch.equal(getattr(fused, n), getattr(pair, n)), f"train_step != grads + apply at {n}"
    compare("three steps", [np.float64(fused.loss.item())] + [getattr(fused, n).cpu().numpy() for n in slots], out[0], out[1], ["loss"] + slots)


@pytest.mark.parametrize("c", [CASES[0], CASES[4]], ids=ident)
def test_chunked_scores_and_top10_against_get_recs(ctx, c):
    case = reference(*c[:3], 1, SCORE_SEED[c[0]])[0]
    chunks = [(0, 32), (32, 64), (64, 70)]
    p64, p32 = (torch.cat([cnmf_ref.Model(case, dt).get_recs(s, e) for s, e in chunks]).numpy().astype(np.float64)
                for dt in (torch.float64, torch.float32))
    tol = bound(p64, p32)
    order = np.argsort(-p64, axis=1, kind="stable")
    top = np.take_along_axis(p64, order, axis=1)
    gaps = top[:, :K] - top[:, 1:K + 1]
    sets, full = gaps[:, K - 1] > 2 * tol, (gaps > 2 * tol).all(1)
    assert sets.mean() >= 0.9                                                                # at most 10 % of the users are left out
    st = device_state(ctx, case)
    got = torch.cat([st.scores(s, e) for s, e in chunks]).cpu().numpy()
    idx = torch.cat([st.recommend(s, e, K)[0] for s, e in chunks]).cpu().numpy()
    print(f"scores {ident(c)}: |kernel - f64| = {distance(got, p64):.3e}, bound {tol:.3e}, ratio {distance(got, p64) / tol:.3f}")
    assert distance(got, p64) <= tol
    assert all(set(idx[r].tolist()) == set(order[r, :K].tolist()) for r in np.flatnonzero(sets))
    assert all(np.array_equal(idx[r], order[r, :K]) for r in np.flatnonzero(full))
    st._image.zero_()                                                                        # a stale image is what gets used ...
    stale = st.scores(0, 32).cpu().numpy()
    assert (stale == stale[:, :1]).all() and not np.array_equal(stale, got[:32])
    st.train_step(*on_device(ctx, case.batch), 0.0)                                          # ... until a step (lr = 0) has touched the state
    assert np.array_equal(st.scores(0, 32).cpu().numpy(), got[:32])
    pu, pi = np.arange(65), (np.arange(65) * 7) % 45                                         # `call` on explicit pairs
    f64, f32 = (m.call(m.V, torch.as_tensor(pu), torch.as_tensor(pi))[0].detach().numpy() for m in (cnmf_ref.Model(case, dt)
                                                                                                  for dt in (torch.float64, torch.float32)))
    fwd = st.forward(*on_device(ctx, (pu.astype(np.int32), pi.astype(np.int32)))).cpu().numpy()
    print(f"forward {ident(c)}: ratio {distance(fwd, f64) / bound(f64, f32):.3f}")
    assert distance(fwd, f64) <= bound(f64, f32)


@pytest.mark.parametrize("F,channels,kernels,strides,word", [(8, (1, 4, 4), (2, 2), (2, 1), "stride"), (8, (2, 4), (2,), (2,), "channels"),
                                                               (8, (1, 65), (2,), (2,), "channels"), (8, (1, 4, 4, 4), (2, 2, 4), (2, 2, 4), "map"),
                                                               (128, (1,) + (2,) * 7, (2,) * 7, (2,) * 7, "layers")])
def test_refusals(ctx, F, channels, kernels, strides, word):
    rs = np.random.RandomState(0)
    w = {"P": rs.rand(70, F), "Q": rs.rand(45, F), "conv": [(rs.rand(k, k, a, b), np.zeros(b)) for k, a, b in zip(kernels, channels, channels[1:])],
         "dense": [(rs.rand(channels[-1], channels[-1]), np.zeros(channels[-1])), (rs.rand(channels[-1], 1), np.zeros(1))]}
    st = ops.ConvNeuMfDeviceState(ctx, w, channels, kernels, strides)
    u = torch.zeros(4, dtype=torch.int32, device=ctx.device)
    for call in (lambda: st.grads(u, u, u), lambda: st.forward(u, u), lambda: st.scores(0, 4)):
        with pytest.raises(_lib.ElliotHipError, match=word):
            call()
