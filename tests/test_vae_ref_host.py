"""CPU: tests/helpers/vae_ref.py (what tests/test_gpu_vae_edges.py holds the Mult-VAE kernels to) against the scalar originals in oracle/,
and the bounds of those GPU tests against the fp32 oracle: a bound that plain fp32 NumPy cannot meet against fp64 on a case's inputs would
say nothing about the kernels."""
import numpy as np
import pytest

from oracle import multi_dae as od
from oracle import multi_vae as ov
from oracle.sampler import philox4x32_10
from tests.helpers import vae_ref as vr

f32 = np.float32


def _scalar_drop_scale(users, I, rate, seed, step):
    """tests/test_gpu_dense.py's drop_scale_matrix: one scalar Philox call per (user, item)."""
    out = np.ones((len(users), I), f32)
    for r, u in enumerate(users):
        for i in range(I):
            x = philox4x32_10(int(u), i, step, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
            uni = f32(x >> 8) * f32(1.0 / 16777216.0)
            out[r, i] = 0.0 if uni < f32(rate) else f32(1.0) / (f32(1.0) - f32(rate))
    return out


@pytest.mark.parametrize("rate", [0.3, 0.5])
def test_vectorised_dropout_mask_equals_the_scalar_philox_bit_for_bit(rate):
    users = np.random.RandomState(3).permutation(5000)[:20]
    for seed, step in ((42, 1), (0xDEADBEEF12345678, 7)):
        got = vr.drop_mask(users, 30, rate, seed, step)
        want = _scalar_drop_scale(users, 30, rate, seed, step)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert 0 < (got == 0).sum() < got.size
    c = np.arange(7)
    words = vr.philox4x32_10(c, c + 1, 0xFFFFFFFF, 5, 0x9E3779B9, 0xFFFFFFFF)
    for t in range(7):
        assert tuple(int(w[t]) for w in words) == philox4x32_10(t, t + 1, 0xFFFFFFFF, 5, 0x9E3779B9, 0xFFFFFFFF)
    assert (vr.drop_mask(users, 30, 0.0, 42, 1) == 1).all()


@pytest.mark.parametrize("name", list(vr.CASES))
def test_make_batch_gives_the_prescribed_counts(name):
    c = vr.case_inputs(name)
    b = c.batch
    assert b.rows.dtype == np.int32 and b.rows.shape == (c.B,) and b.rows.min() >= 0 and b.rows.max() < c.U
    assert set(np.unique(b.X).tolist()) <= {0.0, 1.0} and b.indptr[-1] == len(b.indices) == int(b.X.sum())
    for u in range(c.U):
        assert np.array_equal(b.indices[b.indptr[u]:b.indptr[u + 1]], np.nonzero(b.X[u])[0])
    cnt = vr.batch_counts(b.indptr, b.indices, b.rows, c.I)
    assert np.array_equal(cnt, c.Xb.sum(0).astype(np.int64))
    for item, n in c.want_counts.items():
        assert cnt[item] == n, (item, int(cnt[item]), n)
    assert c.Xb[c.B - 1, c.I - 1] == 1
    others = np.delete(cnt, list(c.want_counts))
    if not name.startswith("dense"):
        assert (others <= vr.W1_LIGHT).any() and (others > 0).any()          # both dW1 kernels have work
    if name.startswith("edge"):
        per_row = c.Xb.sum(1)
        assert sorted(np.nonzero(per_row == 0)[0].tolist()) == sorted(c.empty)
        assert (c.Xb[per_row > 0, 0] == 1).all()
        users, reps = np.unique(b.rows, return_counts=True)
        assert sorted(reps.tolist())[-2:] == [1, 2] and b.rows[c.dup[0]] == b.rows[c.dup[1]]
    if name.startswith("cap"):
        assert c.pos17.min() >= 1024 and c.pos16.min() < 1024 <= c.pos16.max()
        assert np.array_equal(np.nonzero(c.Xb[:, 2])[0], c.pos17) and np.array_equal(np.nonzero(c.Xb[:, 1])[0], c.pos16)


def test_ref_grads_is_the_oracle_in_the_device_layout_scaled_to_the_global_batch():
    for name in ("edge-vae-r0.5", "edge-dae-r0.5"):
        c, step, eps, n_global, drop = vr.run_inputs(name, "plain")
        loss, g = vr.ref_grads(c.w, c.Xb, eps, vr.ANNEAL, drop, c.B, c.dae)
        loss2, g2 = vr.ref_grads(c.w, c.Xb, eps, vr.ANNEAL, drop, 2 * c.B, c.dae)
        assert g["W1"].dtype == np.float64 and abs(loss2 - loss / 2) <= 1e-15 * abs(loss)
        for k in vr.ORDER:
            assert np.allclose(g2[k], g[k] / 2, rtol=1e-14, atol=0)
        if c.dae:
            cc = od.forward(c.w, c.Xb, drop, dtype=np.float64)
            o, want = od.gradients(c.w, cc), od.loss_from(cc)
            assert np.array_equal(g["Wmv"], o["Wm"]) and np.array_equal(g["bmv"], o["bm"])
        else:
            cc = ov.forward(c.w, c.Xb, eps, drop, dtype=np.float64)
            o, want = ov.gradients(c.w, cc, vr.ANNEAL), ov.loss_from(cc, vr.ANNEAL)
            assert np.array_equal(g["Wmv"][:, :c.L], o["Wm"]) and np.array_equal(g["Wmv"][:, c.L:], o["Wv"])
            assert np.array_equal(g["bmv"], np.concatenate([o["bm"], o["bv"]]))
        assert loss == want and np.array_equal(g["W1"], o["W1"]) and np.array_equal(g["b4"], o["b4"])
        # the untouched item's row of gW1 is zero
        assert (g["W1"][3] == 0).all()


@pytest.mark.parametrize("name", [n for n, c in vr.CASES.items() if c["rate"] > 0])
def test_dropout_leaves_every_prescribed_row_of_gw1_something_to_sum(name):
    """At step 1 the one entry of the last item is kept (its row of gW1 is not trivially zero), and the 16- and 17-row items have
    dropped and kept entries alike."""
    c, step, eps, n_global, drop = vr.run_inputs(name, "plain")
    assert step == 1 and drop[c.B - 1, c.I - 1] != 0
    for item, pos in ((1, c.pos16), (2, c.pos17)):
        kept = int((drop[pos, item] != 0).sum())
        assert 0 < kept < len(pos), (item, kept)
    assert np.abs(vr.run_reference(name, "plain")[1]["W1"][c.I - 1]).max() > 0


def test_a_wrong_row_of_a_rare_item_passes_the_tensor_bound_and_fails_its_row_bound():
    """Why the rows are checked one by one: the 17-row item's row of gW1 off by 5e-5 of its own size is inside 2e-5 of the tensor's
    largest entry (the item in every row sets that), and 2.5 times outside 2e-5 of the row's."""
    c = vr.case_inputs("edge-vae-r0.5")
    _, g64 = vr.run_reference("edge-vae-r0.5", "plain")
    bad = {k: np.array(v) for k, v in g64.items()}
    bad["W1"][c.items.n17] *= 1 + 5e-5
    v = {what: (err, bound) for what, err, bound, _ in vr.grad_violations(bad, g64, (c.items.n17,))}
    assert 0 < v["W1"][0] <= v["W1"][1]
    assert v[f"W1[{c.items.n17}]"][0] > 2 * v[f"W1[{c.items.n17}]"][1]


@pytest.mark.parametrize("name,variant", vr.RUNS)
def test_the_fp32_oracle_meets_the_gpu_bounds_on_every_case(name, variant):
    """The bounds of the GPU cases are meaningful on their inputs: plain fp32 NumPy against fp64 stays inside the loss bound, the
    tensor-wide gradient bounds and the per-row bounds of gW1.  (Prints the margins: error / bound.)"""
    c, step, eps, n_global, drop = vr.run_inputs(name, variant)
    loss64, g64 = vr.run_reference(name, variant)
    loss32, g32 = vr.ref_grads(c.w, c.Xb, eps, vr.ANNEAL, drop, n_global, c.dae, dtype=np.float32)
    assert g32["W1"].dtype == np.float32
    lm = abs(float(loss32) - loss64) / (vr.LOSS_RTOL * abs(loss64))
    it = c.items
    v = vr.grad_violations(g32, g64, (it.none, it.last, it.n16, it.n17))
    print(name, variant, "loss margin %.3g tensor margin %.3g row margin %.3g" % (lm, max(m for _, _, _, m in v[:8]), max(m for _, _, _, m in v[8:])))
    assert lm <= 1, (loss32, loss64)
    for what, err, bound, m in v:
        assert err <= bound, (what, err, bound)
    assert (g64["W1"][it.none] == 0).all() and (g32["W1"][it.none] == 0).all()
    assert np.abs(g64["W1"][it.n17]).max() > 0 and np.abs(g64["W1"][it.every]).max() > 0


def test_adam_restatement_is_the_oracles_dense_adam():
    """adam_f32 on the oracle's own gradients against MultiDAEOracle.train_step: identical bits in every variable and slot, two steps."""
    c = vr.case_inputs("edge-dae-r0")
    orc = od.MultiDAEOracle(c.w, 0.001)
    th = {k: np.array(c.w[k], dtype=f32) for k in od.NAMES}
    m, v = {k: np.zeros_like(a) for k, a in th.items()}, {k: np.zeros_like(a) for k, a in th.items()}
    for t in (1, 2):
        g = od.gradients(orc.w, od.forward(orc.w, c.Xb))
        orc.train_step(c.Xb)
        for k in od.NAMES:
            th[k], m[k], v[k], _ = vr.adam_f32(th[k], g[k].astype(f32), m[k], v[k], ov.adam_lr_t(0.001, t))
            assert th[k].dtype == np.float32
            assert np.array_equal(th[k], orc.w[k]) and np.array_equal(m[k], orc.m[k]) and np.array_equal(v[k], orc.v[k]), (t, k)
