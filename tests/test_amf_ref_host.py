"""Host: the AMF restatement (tests/helpers/amf_ref.py) pinned to tests/golden/amf_ref.npz -- what the reference's unmodified
AMF_model.py computes under the tensorflow stand-in (scripts/gen_golden_amf.py) -- and to the BPR-MF oracle where the two must agree.

Tolerance as everywhere for AMF: per array 4 x |float32 run - float64 run| of the restatement, floored at one float32 ulp of the
array's largest magnitude; the fixture is a float32 evaluation of the same function in another order.
"""
import numpy as np
import pytest
import torch

from oracle import bprmf_batch
from tests.helpers import amf_ref


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("amf_ref.npz")
    l_w, l_b, eps, l_adv, eps_iter, nb_iter = z["hyper"].tolist()
    hyper = dict(l_w=l_w, l_b=l_b, eps=eps, l_adv=l_adv)
    return z, hyper, eps_iter, int(nb_iter), (z["u"], z["i"], z["j"]), (z["u2"], z["i2"], z["j2"])


def runs(z, hyper, fn, **delta):
    """fn(model) evaluated by the float64 and the float32 restatement: ([arrays], [arrays]), and the models."""
    out, models = [], []
    for dt in (torch.float64, torch.float32):
        m = amf_ref.Model(z["Gu"], z["Gi"], z["Bi"], hyper["l_w"], hyper["l_b"], hyper["eps"], hyper["l_adv"], dt, **delta)
        out.append([np.asarray(a) for a in fn(m)])
        models.append(m)
    amf_ref.check_case(models)
    return out


def check(what, golden, pair):
    r64, r32 = pair
    for k, (g, a, b) in enumerate(zip(golden, r64, r32)):
        tol, dist = amf_ref.bound(a, b), amf_ref.distance(g, a)
        assert dist <= tol, f"{what}[{k}]: |fixture - f64| = {dist:.3e} > {tol:.3e}"


def test_fgsm_and_msap_perturbations(fx):
    z, hyper, eps_iter, nb_iter, batch, _ = fx

    def fgsm(m):
        m.build_perturbation(batch)
        return m.dGu.numpy(), m.dGi.numpy()

    def msap(m):
        m.build_msap_perturbation(batch, eps_iter, nb_iter)
        return m.dGu.numpy(), m.dGi.numpy()
    check("fgsm", [z["fgsm_dGu"], z["fgsm_dGi"]], runs(z, hyper, fgsm))
    check("msap", [z["msap_dGu"], z["msap_dGi"]], runs(z, hyper, msap))
    touched_u, touched_i = np.unique(batch[0]), np.unique(np.concatenate(batch[1:]))
    for d, rows, n in ((z["fgsm_dGu"], touched_u, amf_ref.U), (z["fgsm_dGi"], touched_i, amf_ref.I)):
        assert not d[np.setdiff1d(np.arange(n), rows)].any()                      # rows outside the batch get 0
        norms = np.linalg.norm(d[rows], axis=1)
        assert np.allclose(norms, hyper["eps"], rtol=1e-5)
    assert np.abs(z["msap_dGu"]).max() <= hyper["eps"] and np.abs(z["msap_dGi"]).max() <= hyper["eps"]


def test_plain_step_reads_theta_plus_delta_and_regularises_the_perturbed_rows(fx):
    z, hyper, _, _, batch, _ = fx
    delta = dict(dGu=z["d0_dGu"], dGi=z["d0_dGi"])
    pair = runs(z, hyper, lambda m: [t.numpy() for t in m.gradients(batch, False)], **delta)
    check("plain step", [z["plain_loss"], z["plain_gBi"], z["plain_gGu"], z["plain_gGi"]], pair)
    # the same step on the plain rows (delta = 0) is a different function: the fixture must tell the two apart
    other = runs(z, hyper, lambda m: [t.numpy() for t in m.gradients(batch, False)])
    assert amf_ref.distance(z["plain_gGu"], other[0][2]) > 100 * amf_ref.bound(pair[0][2], pair[1][2])
    assert hyper["l_w"] > 0


def test_adversarial_step_loss_and_the_delta_it_leaves(fx):
    z, hyper, _, _, batch, _ = fx
    delta = dict(dGu=z["d0_dGu"], dGi=z["d0_dGi"])

    def adv(m):
        loss = m.gradients(batch, True)[0]
        return loss.numpy(), m.dGu.numpy(), m.dGi.numpy()
    check("adversarial step", [z["adv_loss"], z["adv_dGu"], z["adv_dGi"]], runs(z, hyper, adv, **delta))
    assert np.array_equal(z["adv_dGu"], z["fgsm_dGu"]) and np.array_equal(z["adv_dGi"], z["fgsm_dGi"])    # FGSM of the same batch


def test_predict_adds_before_it_multiplies(fx):
    z, hyper, _, _, batch, _ = fx
    delta = dict(dGu=z["fgsm_dGu"], dGi=z["fgsm_dGi"])
    check("predict", [z["predict_adv"], z["predict_clean"]],
          runs(z, hyper, lambda m: (m.predict(3, 20, True).numpy(), m.predict(3, 20, False).numpy()), **delta))


def test_with_delta_zero_a_plain_step_is_bprmf_batchs(fx):
    z, hyper, _, _, batch, _ = fx
    m = amf_ref.Model(z["Gu"], z["Gi"], z["Bi"], hyper["l_w"], hyper["l_b"], hyper["eps"], hyper["l_adv"], torch.float64)
    loss, gB, gU, gI = (t.numpy() for t in m.gradients(batch, False))
    u, i, j = (np.asarray(b) for b in batch)
    f64 = np.float64
    wB, wU, wI = bprmf_batch.gradients(z["Gu"].astype(f64), z["Gi"].astype(f64), z["Bi"].astype(f64), u, i, j, hyper["l_w"], hyper["l_b"], f64)
    assert np.abs(gB - wB).max() < 1e-12 and np.abs(gU - wU).max() < 1e-12 and np.abs(gI - wI).max() < 1e-12
    assert abs(loss - bprmf_batch.forward_loss(z["Gu"], z["Gi"], z["Bi"], u, i, j, hyper["l_w"], hyper["l_b"], f64)) < 1e-9


def test_adam_of_the_restatement_is_the_oracles_sparse_apply(fx):
    z, hyper, _, _, batch, _ = fx
    m = amf_ref.Model(z["Gu"], z["Gi"], z["Bi"], hyper["l_w"], hyper["l_b"], hyper["eps"], hyper["l_adv"], torch.float32)
    _, gB, gU, gI = (t.numpy().copy() for t in amf_ref.Model(z["Gu"], z["Gi"], z["Bi"], hyper["l_w"], hyper["l_b"], hyper["eps"],
                                                          hyper["l_adv"], torch.float32).gradients(batch, True))
    m.train_step(batch, True, 0.01)
    th, mm, vv = z["Gu"].copy(), np.zeros_like(z["Gu"]), np.zeros_like(z["Gu"])
    bprmf_batch.adam_tf_sparse_apply(th, mm, vv, gU, 0.01, 1)
    assert np.array_equal(m.Gu.numpy(), th) and m.step == 1
    untouched = np.setdiff1d(np.arange(amf_ref.I), np.concatenate(batch[1:]))
    assert np.array_equal(m.Gi.numpy()[untouched], z["Gi"][untouched])           # g = 0, m = v = 0: the row stays


def test_a_case_that_breaks_the_promise_is_rejected():
    case = amf_ref.make_case(7, 65)
    m = amf_ref.Model(case.Gu, case.Gi, case.Bi, 0.0, case.l_b, case.eps, case.l_adv)
    m.xs.append(np.array([-80.0005]))
    with pytest.raises(amf_ref.CaseRejected):
        amf_ref.check_case([m])
    m.xs[-1] = np.array([-80.5])
    with pytest.raises(amf_ref.CaseRejected):
        amf_ref.check_case([m])
    m.xs.pop()
    m.norms.append(np.array([0.0, 5e-4]))
    with pytest.raises(amf_ref.CaseRejected):
        amf_ref.check_case([m])
