#!/usr/bin/env python
"""Run the reference's UNMODIFIED adversarial/AMF/AMF_model.py on the `tensorflow` stand-in (oracle/tf_shim) and write
tests/golden/amf_ref.npz.  TEST INFRASTRUCTURE.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_amf.py --reference <elliot v0.3.1 checkout> [--out tests/golden]

Nothing under oracle/ changes: the one symbol the stand-in lacks, tf.stop_gradient, is assigned onto the module here, at run time.

What is recorded is what the stand-in executes faithfully.  Its tape hands back only the gathered part of the gradient of a
variable that was gathered directly anywhere under the tape; the adversarial train_step reads Gu / Gi both directly and through
Gu + Delta_Gu, so its tape.gradient output under the stand-in is NOT the reference's and is not recorded.  Recorded:
  * Delta after build_perturbation and after build_msap_perturbation (3 rounds);
  * loss and gradients of a plain train_step with a non-zero Delta in place -- every table read is then on a sum, which pins that
    the "clean" pass reads theta + Delta and that the regulariser reads the perturbed rows;
  * the loss of an adversarial train_step and the Delta it leaves, apply_gradients stubbed out;
  * predict(adversarial=True / False).
As with every stand-in fixture, this pins the restatement's reading of the FILE, nothing about TensorFlow's library behaviour.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


class Recorder:
    """Stands where the model's optimiser stood: keeps what apply_gradients was handed, changes nothing."""

    def __init__(self):
        self.grads = None

    def apply_gradients(self, grads_and_vars):
        self.grads = [g for g, _ in grads_and_vars]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True                              # nothing may be written under the reference checkout
    sys.path.insert(0, os.path.join(REPO, "oracle", "tf_shim"))  # `import tensorflow` -> the stand-in
    sys.path.insert(1, REPO)
    import numpy as np
    import tensorflow as tf
    import torch
    assert "shim" in tf.__version__
    tf.stop_gradient = lambda x: tf.Tensor(tf._raw(x).detach())
    from oracle.gen_golden_tf import load_by_path
    from tests.helpers import amf_ref
    mod = load_by_path(args.reference, "elliot/recommender/adversarial/AMF/AMF_model.py", "ref_amf_model")

    case = amf_ref.make_case(7, 65)
    l_w, l_b, eps, l_adv, nb_iter = 0.05, case.l_b, case.eps, case.l_adv, 3
    eps_iter = 2.5 * eps / nb_iter
    batch = tuple(np.asarray(b, np.int64) for b in case.batch)
    batch2 = tuple(np.asarray(b, np.int64) for b in amf_ref.make_case(7, 65, second=True).batch)

    def model():
        m = mod.AMF_model(case.F, 0.001, l_w, l_b, eps, l_adv, amf_ref.U, amf_ref.I, 42)
        m._Gu.assign(case.Gu), m._Gi.assign(case.Gi), m._Bi.assign(case.Bi)
        m._optimizer = Recorder()
        return m

    def dense(g, like):
        if isinstance(g, tf.IndexedSlices):
            return torch.zeros(like.shape, dtype=g.values.dtype).index_add_(0, g.indices, g.values).numpy()
        return g.numpy()

    out = {"Gu": case.Gu, "Gi": case.Gi, "Bi": case.Bi, "u": batch[0], "i": batch[1], "j": batch[2], "u2": batch2[0], "i2": batch2[1],
           "j2": batch2[2], "hyper": np.array([l_w, l_b, eps, l_adv, eps_iter, nb_iter], np.float64)}
    m = model()
    m.build_perturbation(batch)
    out["fgsm_dGu"], out["fgsm_dGi"] = m._Delta_Gu.numpy(), m._Delta_Gi.numpy()
    out["predict_adv"], out["predict_clean"] = m.predict(3, 20, True).numpy(), m.predict(3, 20, False).numpy()
    m = model()
    m.build_msap_perturbation(batch, eps_iter, nb_iter)
    out["msap_dGu"], out["msap_dGi"] = m._Delta_Gu.numpy(), m._Delta_Gi.numpy()
    # a plain step on `batch` with the FGSM perturbation of `batch2` in place
    m = model()
    m.build_perturbation(batch2)
    out["d0_dGu"], out["d0_dGi"] = m._Delta_Gu.numpy(), m._Delta_Gi.numpy()
    out["plain_loss"] = np.float64(float(m.train_step(batch, False)))
    gB, gU, gI = m._optimizer.grads
    out["plain_gBi"], out["plain_gGu"], out["plain_gGi"] = dense(gB, case.Bi), dense(gU, case.Gu), dense(gI, case.Gi)
    # an adversarial step from the same state: the loss, and the perturbation it leaves
    m = model()
    m.build_perturbation(batch2)
    out["adv_loss"] = np.float64(float(m.train_step(batch, True)))
    out["adv_dGu"], out["adv_dGi"] = m._Delta_Gu.numpy(), m._Delta_Gi.numpy()
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "amf_ref.npz"), **out)
    print("wrote", os.path.join(args.out, "amf_ref.npz"), {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
