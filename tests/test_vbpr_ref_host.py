"""Host: the VBPR restatement (tests/helpers/vbpr_ref.py) pinned to tests/golden/vbpr_ref.npz -- what the reference's unmodified
VBPR_model.py computes under the tensorflow stand-in (scripts/gen_golden_vbpr.py).

Tolerance as for AMF: per array 4 x |float32 run - float64 run| of the restatement, floored at one float32 ulp of the array's
largest magnitude (amf_ref.bound); the fixture is a float32 evaluation of the same function in another order.  The fixture must also
tell the function from its neighbours: a restatement without the / 10 on the negative bias, with l_e once per sample, or without
l_w on Tu misses it by more than 100 x the bound.
"""
import numpy as np
import pytest
import torch

from oracle import bprmf_batch
from tests.helpers import vbpr_ref

NAMES = vbpr_ref.NAMES


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("vbpr_ref.npz")
    l_w, l_b, l_e, lr = z["hyper"].tolist()
    return z, dict(l_w=l_w, l_b=l_b, l_e=l_e), lr, (z["u"], z["i"], z["j"]), (z["u2"], z["i2"], z["j2"])


def model(z, hyper, dtype, variant=None):
    return vbpr_ref.Model(z["Gu"], z["Gi"], z["Bi"], z["Tu"], z["E"], z["Bp"], z["feat"], hyper["l_w"], hyper["l_b"], hyper["l_e"],
                          dtype, variant)


def runs(z, hyper, fn, variant=None):
    """fn(model) evaluated by the float64 and the float32 restatement: [arrays], [arrays]."""
    out, models = [], []
    for dt in (torch.float64, torch.float32):
        m = model(z, hyper, dt, variant)
        out.append([np.asarray(a) for a in fn(m)])
        models.append(m)
    vbpr_ref.check_case(models)
    return out


def check(what, golden, pair):
    r64, r32 = pair
    assert len(golden) == len(r64)
    for k, (g, a, b) in enumerate(zip(golden, r64, r32)):
        tol, dist = vbpr_ref.bound(a, b), vbpr_ref.distance(np.asarray(g).reshape(a.shape), a)
        assert dist <= tol, f"{what}[{k}]: |fixture - f64| = {dist:.3e} > {tol:.3e}"


def grads_of(batch):
    return lambda m: [t.numpy() for t in m.gradients(batch)]


def test_loss_and_the_six_gradients(fx):
    z, hyper, _, batch, _ = fx
    check("train_step", [z["loss"]] + [z["g" + n] for n in NAMES], runs(z, hyper, grads_of(batch)))
    touched_u, touched_i = np.unique(batch[0]), np.unique(np.concatenate(batch[1:]))
    assert not z["gGu"][np.setdiff1d(np.arange(vbpr_ref.U), touched_u)].any()
    assert not z["gTu"][np.setdiff1d(np.arange(vbpr_ref.U), touched_u)].any()
    for g in (z["gGi"], z["gBi"]):
        assert not g[np.setdiff1d(np.arange(vbpr_ref.I), touched_i)].any()          # rows outside the batch get no gradient
    assert z["gE"].all() and z["gBp"].all()                                          # E and Bp are dense


@pytest.mark.parametrize("variant,array", [("neg_bias_full", "Bi"), ("l_e_per_sample", "E"), ("l_e_per_sample", "Bp"),
                                           ("no_l_w_on_Tu", "Tu")])
def test_the_fixture_tells_the_function_from_its_neighbours(fx, variant, array):
    z, hyper, _, batch, _ = fx
    assert hyper["l_w"] > 0 and hyper["l_b"] > 0 and hyper["l_e"] > 0
    k = 1 + NAMES.index(array)
    true64, true32 = runs(z, hyper, grads_of(batch))
    other64, _ = runs(z, hyper, grads_of(batch), variant)
    tol = vbpr_ref.bound(true64[k], true32[k])
    gold = np.asarray(z["g" + array]).reshape(true64[k].shape)
    assert vbpr_ref.distance(gold, true64[k]) <= tol
    assert vbpr_ref.distance(gold, other64[k]) > 100 * tol, f"{variant}: the fixture's g{array} does not tell the neighbour apart"


def test_variables_after_two_steps_and_the_losses(fx):
    z, hyper, lr, batch, batch2 = fx

    def two(m):
        l1 = m.train_step(batch, lr)
        l2 = m.train_step(batch2, lr)
        return [l1.numpy(), l2.numpy()] + [getattr(m, n).numpy() for n in NAMES]
    check("two steps", [z["loss_1"], z["loss_2"]] + [z["after_" + n] for n in NAMES], runs(z, hyper, two))
    assert float(z["loss_1"]) == float(z["loss"])


def test_predict_item_batch_block(fx):
    z, hyper, lr, batch, batch2 = fx
    s, e, i0, i1 = z["block"].tolist()

    def block(m):
        for n in NAMES:
            getattr(m, n).copy_(torch.as_tensor(z["after_" + n], dtype=m.dtype).reshape(getattr(m, n).shape))
        return [m.predict_item_batch(s, e, i0, i1, z["feat"][i0:i1 + 1]).numpy(), m.predict_all()[s:e, i0:i1 + 1].numpy()]
    check("predict_item_batch", [z["predict"], z["predict"]], runs(z, hyper, block))
    assert z["predict"].shape == (e - s, i1 - i0 + 1)


def test_zero_features_make_the_step_bprmf_batchs(fx):
    z, hyper, _, batch, _ = fx
    m = vbpr_ref.Model(z["Gu"], z["Gi"], z["Bi"], z["Tu"], z["E"], z["Bp"], np.zeros_like(z["feat"]), hyper["l_w"], hyper["l_b"], 0.0)
    loss, gB, gU, gI, gT, gE, gBp = (t.numpy() for t in m.gradients(batch))
    u, i, j = (np.asarray(b) for b in batch)
    f64 = np.float64
    wB, wU, wI = bprmf_batch.gradients(z["Gu"].astype(f64), z["Gi"].astype(f64), z["Bi"].astype(f64), u, i, j, hyper["l_w"], hyper["l_b"], f64)
    assert np.abs(gB - wB).max() < 1e-12 and np.abs(gU - wU).max() < 1e-12 and np.abs(gI - wI).max() < 1e-12
    assert not gE.any() and not gBp.any()
    assert np.abs(gT - hyper["l_w"] * np.bincount(u, minlength=vbpr_ref.U)[:, None] * z["Tu"]).max() < 1e-12     # l_w per occurrence


def test_adam_moves_every_row_and_steps_the_dense_pair_in_delta_form(fx):
    z, hyper, lr, batch, _ = fx
    m = model(z, hyper, torch.float32)
    _, gB, gU, gI, gT, gE, gBp = (t.numpy().copy() for t in model(z, hyper, torch.float32).gradients(batch))
    m.train_step(batch, lr)
    th, mm, vv = z["Tu"].copy(), np.zeros_like(z["Tu"]), np.zeros_like(z["Tu"])
    bprmf_batch.adam_tf_sparse_apply(th, mm, vv, gT, lr, 1)
    assert np.array_equal(m.Tu.numpy(), th) and m.step == 1
    th, mm, vv = z["E"].copy(), np.zeros_like(z["E"]), np.zeros_like(z["E"])
    vbpr_ref.adam_dense_apply(th, mm, vv, gE, lr, 1)
    assert np.array_equal(m.E.numpy(), th)
    untouched = np.setdiff1d(np.arange(vbpr_ref.I), np.concatenate(batch[1:]))
    assert np.array_equal(m.Gi.numpy()[untouched], z["Gi"][untouched])           # g = 0, m = v = 0: the row stays
