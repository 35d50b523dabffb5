"""GPU: the gradient sums of the point-wise factor models (elliot_amd/csrc/el_pwmf.hip, el_segcombine.h) BEFORE the optimiser, through
PwmfDeviceState.grads, against fp64 (tests/helpers/pwcml_ref.py; tests/test_pwcml_ref_host.py checks helper, budgets and bounds without a GPU).
  exact cases      MF / FunkSVD on dyadic inputs with n_global a power of two: every fp32 product and partial sum is representable in any order
                   of summation (the helper asserts the 2^24 budget per case), so gGu, gGi, gBu, gBi and the loss must have the fp64 BITS
    layouts        segments planted against the chunk borders (users: 4 positions, items: 16), confirmed by assert_layout before every call:
                   plain stores next to a border, head / tail pieces of one position, a middle piece, two cut rows in one chunk, lpt - 2 .. lpt + 1
                   continuations (k_seg_combine against the long list), 255 / 256 / 257 / 513 (the passes of the long kernel's search), the first
                   row cut, the last row cut and ending with the data, n % chunk != 0, n < chunk, n = 1; both sides at once and each alone
    lane classes   F with CPL 1, 2, 4 on the vector and the scalar path (k_pw_fwd, k_pw_seg's SUB = 4 / 2 / 1 staging, both combines;
                   F = 1024 fills k_seg_combine_long's s_red), and k_pw_predict at the same F
  refused sizes    F = 257 (scalar) and 1028 (vector) are turned down before anything is launched
  bounded kinds    PMF and LogisticMF against the forward-error bound derived in the helper; the largest |got - ref| / bound is printed
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
NAMES = ("Gu", "Gi", "Bu", "Bi")


def _dev(ctx, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def _state(ctx, w, kind="mse", alpha=0.0, l_w=0.0):
    return ops.PwmfDeviceState(ctx, w["Gu"], w["Gi"], w.get("Bu"), w.get("Bi"), kind=kind, optimizer="adagrad", alpha=alpha, l_w=l_w)


def _bits_equal(got, ref):
    """fp32 result against an fp64 reference that must itself be an fp32 number; -0 and +0 are one value."""
    ref32 = np.asarray(ref, f64).astype(f32)
    assert np.array_equal(ref32.astype(f64), ref), "the reference is not representable: not an exact case"
    return np.array_equal((np.asarray(got, f32) + f32(0)).view(np.uint32), (ref32 + f32(0)).view(np.uint32))


def _grads(ctx, st, c, side, n_global):
    for k in NAMES:                                                # accumulators start zero, as the contract has it
        t = getattr(st, "g" + k)
        if t is not None:
            t.zero_()
    st.pop_loss()
    st.grads(_dev(ctx, c.u, np.int32), _dev(ctx, c.i, np.int32), _dev(ctx, c.y, np.float32), n_global=n_global, side=side)
    return st.pop_loss(), {k: cpu(getattr(st, "g" + k)) for k in c.w}


def _check_exact(ctx, c, tag, sides=("both", "users", "items")):
    pu, pi = c.plans
    R.assert_layout(c.u, pu), R.assert_layout(c.i, pi)             # the layout is the docstring's, or the test fails here
    assert c.budget < R.BUDGET
    st = _state(ctx, c.w)
    for side in sides:
        want_loss, want = R.pw_ref(c.w, "mse", c.u, c.i, c.y, c.n_global, side=side)
        loss, got = _grads(ctx, st, c, side, c.n_global)
        assert loss == want_loss, (tag, side, loss, want_loss)
        for k in want:
            if not _bits_equal(got[k], want[k]):
                bad = np.nonzero((got[k].astype(f64) != want[k]).reshape(len(want[k]), -1).any(1))[0]
                plan = pu if k in ("Gu", "Bu") else pi
                named = {v: n for n, v in plan.names.items()}
                raise AssertionError((tag, side, k, "rows", bad[:12].tolist(), [named.get(int(r)) for r in bad[:12]],
                                      got[k][bad[0]].ravel()[:4].tolist(), want[k][bad[0]].ravel()[:4].tolist()))
    return st


_LAYOUT_CASES = [(name, F, bias) for name in R.LAYOUTS for F in R.PW_LAYOUT_F for bias in (False, True) if not (name.startswith("long") and F != 8)]


@pytest.mark.parametrize("name,F,bias", _LAYOUT_CASES)
def test_planted_layouts_have_the_fp64_bits(ctx, name, F, bias):
    c = R.pw_exact_case(name, F, bias)
    _check_exact(ctx, c, (name, F, bias))


def test_rows_outside_the_batch_stay_bit_zero(ctx):
    """The tables hold rows past the batch's: their accumulators are never written."""
    c = R.pw_exact_case("small", 8, True)
    rs = np.random.RandomState(2)
    w = {k: np.concatenate([v, R.dyadic(rs, (9,) + v.shape[1:])]) for k, v in c.w.items()}
    st = _state(ctx, w)
    _, want = R.pw_ref(w, "mse", c.u, c.i, c.y, c.n_global)
    for k in NAMES:
        getattr(st, "g" + k).zero_()
    st.grads(_dev(ctx, c.u, np.int32), _dev(ctx, c.i, np.int32), _dev(ctx, c.y, np.float32), n_global=c.n_global)
    for k in NAMES:
        got = cpu(getattr(st, "g" + k))
        assert _bits_equal(got, want[k]) and not got[-9:].view(np.uint32).any(), k


@pytest.mark.parametrize("F", R.PW_CLASS_F)
def test_lane_classes_have_the_fp64_bits(ctx, F):
    c = R.pw_exact_case("class", F, True)
    pu, pi = c.plans
    L = R.lanes(F)[1]
    conts_u, conts_i = R.assert_layout(c.u, pu), R.assert_layout(c.i, pi)
    assert conts_u[pu.names["long"]] == conts_i[pi.names["long"]] == L and conts_u[pu.names["short_cut"]] == 1
    st = _check_exact(ctx, c, ("class", F), sides=("both",))
    out = cpu(st.forward(_dev(ctx, c.u, np.int32), _dev(ctx, c.i, np.int32)))          # k_pw_predict
    want = R.pw_coef(c.w, "mse", c.u, c.i, c.y, c.n_global)[0]
    assert _bits_equal(out, want), (F, int((out.astype(f64) != want).sum()))


@pytest.mark.parametrize("F", R.PW_REFUSED_F)
def test_sizes_past_four_chunks_per_lane_are_refused_before_any_launch(ctx, F):
    rs = np.random.RandomState(F)
    w = {"Gu": R.dyadic(rs, (5, F)), "Gi": R.dyadic(rs, (6, F)), "Bu": R.dyadic(rs, (5,)), "Bi": R.dyadic(rs, (6,))}
    st = _state(ctx, w)
    u, i, y = _dev(ctx, [0, 1, 4, 4], np.int32), _dev(ctx, [5, 0, 2, 2], np.int32), _dev(ctx, [1, 0, 1, 0], np.float32)
    for k in NAMES:
        getattr(st, "g" + k).fill_(3.0)
    st.loss.fill_(7.0)
    with pytest.raises(ElliotHipError, match="too large"):
        st.grads(u, i, y)
    out = torch.full((4,), 5.0, dtype=torch.float32, device=ctx.device)
    with pytest.raises(ElliotHipError, match="too large"):
        st.forward(u, i, out=out)
    torch.cuda.synchronize()
    assert all(bool((getattr(st, "g" + k) == 3.0).all()) for k in NAMES) and float(st.loss.item()) == 7.0 and bool((out == 5.0).all())


@pytest.mark.parametrize("model", list(R.PW_BOUNDED_KINDS))
@pytest.mark.parametrize("layout,F", R.pw_bounded_cases())
def test_bounded_kinds_stay_inside_the_derived_bound(ctx, layout, F, model):
    """PMF (sigmoid) and LogisticMF (softplus, alpha = 0.5, l_w = 2^-5, items then users) on the cut-row layouts and on F = 8, 65, 260, 516.
    The bound is the helper's forward error analysis (expf / log1pf assumed within 2 ulp), not a fitted tolerance."""
    c = R.pw_bounded_case(layout, F, model)
    pu, pi = c.plans
    R.assert_layout(c.u, pu), R.assert_layout(c.i, pi)
    st = _state(ctx, c.w, kind=c.kind, alpha=c.alpha, l_w=c.l_w)
    for side in c.sides:
        want_loss, want = R.pw_ref(c.w, c.kind, c.u, c.i, c.y, c.n_global, side=side, alpha=c.alpha, l_w=c.l_w)
        loss_bound, bound = R.pw_bound(c.w, c.kind, c.u, c.i, c.y, c.n_global, side=side, alpha=c.alpha, l_w=c.l_w)
        loss, got = _grads(ctx, st, c, side, c.n_global)
        ratios = {k: R.bound_ratio(got[k], want[k], bound[k]) for k in want}
        ratios["loss"] = abs(loss - want_loss) / loss_bound
        print("bound ratio", model, layout, F, side, " ".join("%s %.3g" % kv for kv in ratios.items()))
        assert max(ratios.values()) <= 1.0, (model, layout, F, side, ratios)
    out = cpu(st.forward(_dev(ctx, c.u, np.int32), _dev(ctx, c.i, np.int32)))
    want = R.pw_coef(c.w, c.kind, c.u, c.i, c.y, c.n_global, c.alpha)[0]
    if c.kind == "mse_sigmoid":
        want = 1.0 / (1.0 + np.exp(-want))
    ratio = float((np.abs(out - want) / R.pw_forward_bound(c.w, c.kind, c.u, c.i)).max())
    print("bound ratio", model, layout, F, "forward %.3g" % ratio)
    assert ratio <= 1.0
