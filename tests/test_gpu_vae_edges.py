"""GPU: the Mult-VAE / Mult-DAE step (elliot_amd/csrc/el_vae.hip) at the edges of its kernels, against oracle/multi_vae.py and
oracle/multi_dae.py evaluated in fp64 (tests/helpers/vae_ref.py; tests/test_vae_ref_host.py checks the helper and the bounds without a GPU).
  k_vae_w1_light / k_vae_w1_rows   items in exactly 16 and 17 batch rows (the hand-over between the two), in every row, in none, in the last
                                   row alone; under dropout, with B no multiple of 64, with the batch means over more rows than the batch has
  presence flags                   cap = 2048 (B = 1100 and 2048): rows at positions >= 1024, a list that straddles 1024
  k_vae_densify + product          B = 2049
  chunks per lane                  H = 4, 260, 516, 772, 1024 -> CPL 1, 2, 3, 4, 4; H = 1024 asks for 64 KiB (k_vae_enc1) and 65 KiB
                                   (k_vae_w1_rows) of dynamic LDS
  k_vae_softmax<false>             I = 203 in the step and in predict; users without a train item
  one-stream backward              option vae_side = 0
  k_adam_apply_oct                 the scalar tails (lengths 203, 14, 7) against an fp32 restatement, m and v bit for bit
Every gradient call starts from a gW1 full of NaN: the step writes every row, zeros for the items the batch does not touch.
"""
import numpy as np
import pytest
import torch

from elliot_amd import ops
from tests.gpu_util import cpu
from tests.helpers import vae_ref as vr

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float("nan")


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _state(ctx, c, max_batch=None):
    """Device state and train matrix of a case, after the prescribed in-batch counts were checked on the host."""
    b = c.batch
    cnt = vr.batch_counts(b.indptr, b.indices, b.rows, c.I)
    for item, n in c.want_counts.items():
        assert cnt[item] == n, (c.name, item, int(cnt[item]), n)
    st = ops.VaeDeviceState(ctx, c.w, max_batch=c.B if max_batch is None else max_batch)
    assert st.dae == c.dae
    return st, ops.DeviceCSR(b.indptr, b.indices, c.I, ctx.device)


def _grads_and_check(ctx, st, csr, name, variant):
    """One st.grads call on a gW1 full of NaN; loss within 1e-4 relative of fp64, each gradient tensor within 2e-5 of its reference's
    largest |entry|, and the rows of gW1 of the 16-, 17-, one- and no-row items each within 2e-5 of THAT row's largest |entry| (the item
    in every row dominates the tensor-wide maximum: a wrong row of a rare item would hide under it)."""
    c, step, eps, n_global, _ = vr.run_inputs(name, variant)
    want_loss, want = vr.run_reference(name, variant)
    st.step = step - 1
    st.g[0].fill_(NAN)
    st.pop_loss()
    st.grads(csr, _dev(ctx, c.batch.rows), vr.ANNEAL, eps=None if eps is None else _dev(ctx, eps), dropout_rate=c.rate,
             dropout_seed=vr.DROP_SEED, n_global=None if n_global == c.B else n_global)
    loss = st.pop_loss()
    got = {k: cpu(t) for k, t in zip(st.ORDER, st.g)}
    it = c.items
    v = vr.grad_violations(got, want, (it.none, it.last, it.n16, it.n17))
    print(name, variant, "loss %.9g want %.9g (%.3g of the bound);" % (loss, want_loss, abs(loss - want_loss) / (vr.LOSS_RTOL * abs(want_loss))),
          " ".join("%s %.3g" % (k, m) for k, _, _, m in v))
    assert not np.isnan(got["W1"]).any(), ("rows of gW1 left unwritten", np.nonzero(np.isnan(got["W1"]).any(1))[0][:10].tolist())
    assert abs(loss - want_loss) <= vr.LOSS_RTOL * abs(want_loss), (loss, want_loss)
    for what, err, bound, _ in v:
        assert err <= bound, (name, variant, what, err, bound)
    assert (got["W1"][it.none] == 0).all()
    return got


# ---- 1. heavy / light boundary, odd widths, empty users ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "nglobal", "oneside", "step2"])
@pytest.mark.parametrize("name", [n for n in vr.CASES if n.startswith("edge")])
def test_step_with_16_and_17_row_items_odd_widths_and_empty_users(ctx, lib_option, name, variant):
    """I = 203, L = 7, B = 150 (no multiple of 4, of 64): item 1 in 16 batch rows (k_vae_w1_light's last), item 2 in 17 (k_vae_w1_rows'
    first), item 0 in every row, item 3 in none, item 202 in the last row alone; three users without items (nrm = 1e6 on the device, a
    zero row in the reference), one user twice.  plain: step 1 with eps; nglobal: batch means over 2 B rows; oneside: the backward pass on
    one stream (the workspace is carved differently); step2: a second call on the same state at step 2 -- another dropout mask --
    without eps."""
    c = vr.case_inputs(name)
    st, csr = _state(ctx, c)
    if variant == "oneside":
        lib_option("vae_side", 0)
    if variant == "step2":
        _grads_and_check(ctx, st, csr, name, "plain")
        if c.rate > 0:
            assert (vr.run_inputs(name, "plain")[4] != vr.run_inputs(name, "step2")[4]).any()
    _grads_and_check(ctx, st, csr, name, variant)


# ---- 2. chunks per lane; the LDS request at H = 1024 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 260, 516, 772, 1024])
def test_step_at_every_chunks_per_lane(ctx, H):
    """H/4 = 1, 65, 129, 193, 256 float4 chunks over 64 lanes: CPL 1, 2, 3, 4 and 4 of k_vae_enc1 / k_vae_w1_light / k_vae_w1_rows, each
    but the first and last with a last chunk that only lane 0 owns.  H = 1024 is the widest layer vae_check admits: k_vae_enc1 takes
    65 536 B and k_vae_w1_rows 66 560 B of dynamic LDS."""
    name = f"cpl-H{H}"
    st, csr = _state(ctx, vr.case_inputs(name))
    _grads_and_check(ctx, st, csr, name, "plain")


# ---- 3. presence flags beyond 1024 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cap-B1100", "cap-B2048"])
def test_step_with_2048_presence_flags(ctx, name):
    """B > 1024: cap = 2048, 128 batch rows per wave of k_vae_w1_rows.  Item 2 is in 17 rows, all at batch positions >= 1024; item 1 in
    the 16 rows 1016 .. 1031; item 0 in every row.  B = 2048 is the largest batch the sparse dW1 takes."""
    st, csr = _state(ctx, vr.case_inputs(name))
    _grads_and_check(ctx, st, csr, name, "plain")


# ---- 4. dense fallback ---------------------------------------------------------------------------------------------------------------------
def test_step_with_the_dense_first_layer_gradient(ctx):
    """B = 2049: dW1 = densified batch^T dh (k_vae_densify + one transposed product) -- the same assertions as the sparse paths."""
    st, csr = _state(ctx, vr.case_inputs("dense-B2049"), max_batch=2049)
    _grads_and_check(ctx, st, csr, "dense-B2049", "plain")


# ---- 5. predict ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge-vae-r0", "edge-dae-r0"])
def test_predict_with_unaligned_rows_and_empty_users(ctx, name):
    """I = 203: k_vae_softmax<false>; the batch holds the three users without items.  log_softmax within 1e-4 of fp64, every row's
    exp sums to 1 within 1e-4, with and (VAE) without eps."""
    c = vr.case_inputs(name)
    st, csr = _state(ctx, c)
    rows = _dev(ctx, c.batch.rows)
    for eps in ((None,) if c.dae else (None, c.eps)):
        st.logits.fill_(NAN)
        pred = cpu(st.predict(csr, rows, eps=None if eps is None else _dev(ctx, eps)))
        ref = vr.ref_predict(c.w, c.Xb, eps, c.dae)
        assert pred.shape == ref.shape == (c.B, c.I)
        err = np.abs(pred - ref).max()
        print(name, "eps" if eps is not None else "no eps", "max |log_softmax - fp64| %.3g" % err)
        assert err < 1e-4
        assert np.abs(np.exp(pred).sum(1) - 1).max() < 1e-4
        assert np.abs(pred[list(c.empty)] - ref[list(c.empty)]).max() < 1e-4


# ---- 6. Adam in isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dae", [False, True])
def test_adam_tails_match_the_fp32_restatement(ctx, dae):
    """k_adam_apply_oct on known slots at I = 203, L = 7: b4 has 203 entries, bmv 14 (VAE) or 7 (DAE) -- 16-byte lanes and a scalar tail.
    g holds zeros, v holds zeros (also where g is zero: the update is m alpha / eps).  Two steps against vae_ref.adam_f32, which rounds
    every operation once to fp32 in the kernel's order.
      m, v   only IEEE fp32 add and multiply, compiled without contraction: bit-equal
      th     update = (m alpha) / (sqrt(v) + eps): the multiply, the square root, the add and the divide may each be off by one rounding
             (2^-24 relative) on the device, so the update differs by at most 4 x 2^-24 |update|; the final th - update rounds once more
             on each side: ulp(th) (of the larger of |th| before and after).  The bound is this derivation, not what a device gives."""
    c = vr.case_inputs("edge-dae-r0" if dae else "edge-vae-r0")
    st = ops.VaeDeviceState(ctx, c.w, max_batch=8)
    assert st.w[7].numel() == 203 and st.w[3].numel() == (7 if dae else 14)
    rs = np.random.RandomState(77)
    host = {"g": [], "m": [], "v": []}
    for k in range(8):
        shape = tuple(st.w[k].shape)
        g = (rs.normal(size=shape) * 1e-3).astype(f32)
        m = (rs.normal(size=shape) * 1e-3).astype(f32)
        v = (rs.uniform(0, 1e-3, size=shape) ** 2).astype(f32)
        g[rs.rand(*shape) < 0.2] = 0
        v[rs.rand(*shape) < 0.2] = 0
        g.reshape(-1)[-1], v.reshape(-1)[-1] = 0, 0                       # the last entry (in the scalar tail): g = 0 and v = 0
        g.reshape(-1)[-2] = 0
        v.reshape(-1)[0] = 0
        for slot, a in (("g", g), ("m", m), ("v", v)):
            host[slot].append(a)
        st.g[k].copy_(_dev(ctx, g)), st.m[k].copy_(_dev(ctx, m)), st.v[k].copy_(_dev(ctx, v))
    th = [cpu(t).copy() for t in st.w]
    m, v = host["m"], host["v"]
    lr = 0.001
    for step in (1, 2):
        st.apply(lr)
        assert st.step == step
        for k, nm in enumerate(st.ORDER):
            want_th, want_m, want_v, upd = vr.adam_f32(th[k], host["g"][k], m[k], v[k], ops.adam_lr_t(lr, step))
            got_th, got_m, got_v = cpu(st.w[k]), cpu(st.m[k]), cpu(st.v[k])
            assert np.array_equal(cpu(st.g[k]).view(np.uint32), host["g"][k].view(np.uint32)), (step, nm)          # apply leaves g alone
            assert np.array_equal(got_m.view(np.uint32), want_m.view(np.uint32)), (step, nm, int((got_m != want_m).sum()))
            assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), (step, nm, int((got_v != want_v).sum()))
            assert np.isfinite(got_th).all()
            bound = 4 * 2.0 ** -24 * np.abs(upd.astype(np.float64)) + np.spacing(np.maximum(np.abs(th[k]), np.abs(want_th))).astype(np.float64)
            err = np.abs(got_th.astype(np.float64) - want_th.astype(np.float64))
            print(step, nm, "th: %d of %d entries differ, worst %.3g of the bound" % (int((err > 0).sum()), err.size, float((err / bound).max())))
            assert (err <= bound).all(), (step, nm, float((err / bound).max()))
            th[k], m[k], v[k] = got_th.copy(), got_m.copy(), got_v.copy()
