"""GPU: Collaborative Metric Learning (elliot_amd/csrc/el_cml.hip, the cml branches of el_bpr_sorted.hip, el_segcombine.h) before the optimiser,
against fp64 (tests/helpers/pwcml_ref.py; tests/test_pwcml_ref_host.py checks helper, budgets and bounds without a GPU).
  forward_de       dyadic tables, l_b = 0: D, E and the regulariser have the fp64 bits at every lane class (CPL 1, 2, 4; vector and scalar rows)
  grads_de         D, E GIVEN on multiples of 1/8, so the hinge and clip memberships are decided on exact ties: pairs with D_a + E_b = margin,
                   margin -+ 1/8, -80, -80 -+ 1/8 (equality is active), runs of equal E and of equal D values, every pair clipped, no pair active,
                   B_all > B with the local triplets at the front and in the middle, B = 1, and B = 2047 against 2048 (float atomics against the
                   sorted segments, one hot positive item cut over more than lpt chunks).  gGu, gGi, gBi and the hinge share: the fp64 bits
  train_step       one step on an exact batch: the loss bit for bit, the accumulators handed back zero
  rescore, items   Gi2 = 2 Gi bit for bit; Bi2 and the re-scored values inside the helper's bound; idx < 0 -> -inf; a list width that leaves the
                   last wave of a workgroup without a row
  refused sizes    F = 257 / 1028 are turned down before anything is launched, on both gradient paths
"""
import numpy as np
import pytest
import torch

from elliot_amd import ops
from elliot_amd._lib import ElliotHipError
from tests.gpu_util import cpu
from tests.helpers import pwcml_ref as R

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
L_W, MARGIN = R.CML_L_W, R.CML_MARGIN


def _ids(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(ctx.device)


def _f(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ctx.device)


def _bits_equal(got, ref):
    ref32 = np.asarray(ref, f64).astype(f32)
    assert np.array_equal(ref32.astype(f64), ref), "the reference is not representable: not an exact case"
    return np.array_equal((np.asarray(got, f32) + f32(0)).view(np.uint32), (ref32 + f32(0)).view(np.uint32))


def _bad_rows(got, ref):
    return np.nonzero((got.astype(f64) != ref).reshape(len(ref), -1).any(1))[0][:12].tolist()


@pytest.mark.parametrize("F", R.CML_FORWARD_F)
def test_forward_de_has_the_fp64_bits(ctx, F):
    c = R.cml_forward_case(F)
    assert c.budget < R.BUDGET
    st = ops.CmlDeviceState(ctx, c.Gu, c.Gi, c.Bi)
    st.pop_loss()
    D, E = st.forward_de(_ids(ctx, c.u), _ids(ctx, c.i), _ids(ctx, c.j), L_W, 0.0)
    wD, wE, reg = R.cml_forward_ref(c.Gu, c.Gi, c.Bi, c.u, c.i, c.j, L_W, 0.0)
    assert _bits_equal(cpu(D), wD) and _bits_equal(cpu(E), wE), (F, _bad_rows(cpu(D), wD))
    assert st.pop_loss() == reg
    assert not cpu(st.gGu).any() and not cpu(st.item_grad_flat).any()
    if F == 36:                                                    # l_b != 0: the negative item's / 10 is not dyadic -- bounded
        l_b = float(f32(0.02))
        st.forward_de(_ids(ctx, c.u), _ids(ctx, c.i), _ids(ctx, c.j), L_W, l_b)
        _, _, reg = R.cml_forward_ref(c.Gu, c.Gi, c.Bi, c.u, c.i, c.j, L_W, l_b)
        bound = R.cml_reg_bound(c.Gu, c.Gi, c.Bi, c.u, c.i, c.j, L_W, l_b)
        got = st.pop_loss()
        print("bound ratio cml regulariser %.3g" % (abs(got - reg) / bound))
        assert abs(got - reg) <= bound


def _run_grads(ctx, c, st=None):
    st = ops.CmlDeviceState(ctx, c.Gu, c.Gi, c.Bi) if st is None else st
    st.gGu.zero_(), st.item_grad_flat.zero_()
    st.pop_loss()
    st.grads_de(_ids(ctx, c.u), _ids(ctx, c.i), _ids(ctx, c.j), L_W, 0.0, MARGIN, _f(ctx, c.D), _f(ctx, c.E), _f(ctx, c.D_all), _f(ctx, c.E_all))
    return st, st.pop_loss(), cpu(st.gGu), cpu(st.gGi), cpu(st.gBi)


@pytest.mark.parametrize("case", R.CML_GRADS_CASES, ids=lambda t: "-".join(str(x) for x in t))
def test_grads_de_has_the_fp64_bits_on_planted_ties(ctx, case):
    F, B, kind, B_all, lo, hot = case
    c = R.cml_grads_case(*case)
    assert c.budget < R.BUDGET and len(c.u) == B
    n_a, m_b, low_a = c.counts
    if kind == "clipped":
        assert not n_a.any() and not m_b.any() and c.hinge == B * len(c.D_all) * (MARGIN + 80.0)
    if kind == "inactive":
        assert not n_a.any() and not m_b.any() and not low_a.any() and c.hinge == 0.0 and c.dGu.any()     # the l_w terms alone
    if B == 2047:                                                  # the atomic kernel's triplets are a prefix of the sorted path's
        big = R.cml_grads_case(F, 2048, kind, B_all, lo, hot)
        assert all(np.array_equal(getattr(c, k), getattr(big, k)[:B]) for k in ("u", "i", "j"))
    _, loss, gGu, gGi, gBi = _run_grads(ctx, c)
    assert loss == c.hinge, (case, loss, c.hinge)
    for name, got, want in (("gGu", gGu, c.dGu), ("gGi", gGi, c.dGi), ("gBi", gBi, c.dBi)):
        assert _bits_equal(got, want), (case, name, _bad_rows(got, want))


@pytest.mark.parametrize("F,B", [(8, 300), (65, 300), (8, 2048), (260, 2048)])
def test_train_step_on_an_exact_batch(ctx, F, B):
    c = R.cml_grads_case(F, B, hot=B >= R.CML_SORTED_FROM)
    assert R.cml_forward_budget(c.Gu, c.Gi, c.Bi, c.u, c.i, c.j, L_W) < R.BUDGET      # the D, E the step computes itself are exact too
    D, E, reg = R.cml_forward_ref(c.Gu, c.Gi, c.Bi, c.u, c.i, c.j, L_W, 0.0)
    want = reg + R.cml_hinge_full(D, E, MARGIN)
    st = ops.CmlDeviceState(ctx, c.Gu, c.Gi, c.Bi)
    st.train_step(_ids(ctx, c.u), _ids(ctx, c.i), _ids(ctx, c.j), 0.01, L_W, 0.0, MARGIN)
    assert st.pop_loss() == want
    assert not cpu(st.gGu).view(np.uint32).any() and not cpu(st.item_grad_flat).view(np.uint32).any()
    assert (cpu(st.Gu) != c.Gu).any() and (cpu(st.Gi) != c.Gi).any()


@pytest.mark.parametrize("F", [1, 63, 64, 65, 200, 1024])
def test_item_side_and_rescore(ctx, F):
    rs = np.random.RandomState(F)
    U, I = 7, 23
    Gu, Gi, Bi = (rs.normal(scale=0.4, size=s).astype(f32) for s in ((U, F), (I, F), (I,)))
    st = ops.CmlDeviceState(ctx, Gu, Gi, Bi)
    Gi2, Bi2 = (cpu(t) for t in st._item_side())
    assert np.array_equal(Gi2.view(np.uint32), (f32(2) * Gi).view(np.uint32))
    g64, b64 = Gi.astype(f64), Bi.astype(f64)
    ratio = np.abs(Bi2 - (b64 - np.sum(g64 * g64, -1))) / R.item_side_bound(g64, b64)
    # three rows of five candidates: 15 waves, the last workgroup's last wave has no row
    idx = rs.randint(0, I, (3, 5)).astype(np.int32)
    idx[0, 1] = idx[2, 4] = -1
    val = cpu(st.rescore(_ids(ctx, idx), 2))
    neg = idx < 0
    assert np.isneginf(val[neg]).all() and np.isfinite(val[~neg]).all()
    it = np.where(neg, 0, idx)
    u64 = Gu.astype(f64)[2:5, None, :]
    ref = b64[it] - np.sum((u64 - g64[it]) ** 2, -1)
    r2 = (np.abs(val - ref) / R.rescore_bound(u64, g64[it], b64[it], F))[~neg]
    print("bound ratio cml F=%d item side %.3g rescore %.3g" % (F, ratio.max(), r2.max()))
    assert ratio.max() <= 1.0 and r2.max() <= 1.0


@pytest.mark.parametrize("F", R.PW_REFUSED_F)
def test_sizes_past_four_chunks_per_lane_are_refused_before_any_launch(ctx, F):
    rs = np.random.RandomState(F)
    Gu, Gi, Bi = R.dyadic(rs, (6, F)), R.dyadic(rs, (9, F)), R.dyadic(rs, (9,))
    st = ops.CmlDeviceState(ctx, Gu, Gi, Bi)
    st.gGu.fill_(3.0), st.item_grad_flat.fill_(3.0), st.loss.fill_(7.0)
    for B in (5, R.CML_SORTED_FROM + 2):
        u, i, j = (_ids(ctx, rs.randint(0, n, B)) for n in (6, 9, 9))
        z = _f(ctx, np.zeros(B))
        with pytest.raises(ElliotHipError, match="too large"):
            st.forward_de(u, i, j, L_W, 0.0)
        with pytest.raises(ElliotHipError, match="too large"):
            st.grads_de(u, i, j, L_W, 0.0, MARGIN, z, z, z, z)
        with pytest.raises(ElliotHipError, match="too large"):
            st.train_step(u, i, j, 0.01, L_W, 0.0, MARGIN)
    torch.cuda.synchronize()
    assert bool((st.gGu == 3.0).all()) and bool((st.item_grad_flat == 3.0).all()) and float(st.loss.item()) == 7.0
    assert np.array_equal(cpu(st.Gu), Gu.astype(f32)) and np.array_equal(cpu(st.Gi), Gi.astype(f32))
