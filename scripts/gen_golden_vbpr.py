#!/usr/bin/env python
"""Run the reference's UNMODIFIED visual_recommenders/VBPR/VBPR_model.py on the `tensorflow` stand-in (oracle/tf_shim) and write
tests/golden/vbpr_ref.npz.  TEST INFRASTRUCTURE.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_vbpr.py --reference <elliot v0.3.1 checkout> [--out tests/golden]

Nothing under oracle/ changes, and VBPR_model.py uses no symbol the stand-in lacks.  Bi, Gu, Gi and Tu are read through
embedding_lookup only and E, Bp directly only, so the stand-in's tape hands back what the file asks for: four IndexedSlices
and two dense gradients.

Recorded -- data only:
  * the inputs (six variables, the feature matrix, two batches, the hyper-parameters);
  * loss and the six gradients of one train_step, apply_gradients stubbed out;
  * the six variables after two train_steps with the model's own optimizer (batch, then batch2);
  * predict_item_batch on a block of users x a block of items after those steps.
`predict` (:98-101) reads self.F, which nothing sets: it cannot run and nothing of it is recorded.
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
    from oracle.gen_golden_tf import load_by_path
    from tests.helpers import vbpr_ref
    mod = load_by_path(args.reference, "elliot/recommender/visual_recommenders/VBPR/VBPR_model.py", "ref_vbpr_model")

    case = vbpr_ref.make_case(7, 5, 33, 65)
    lr = 0.01
    batch = tuple(np.asarray(b, np.int64) for b in case.batch)
    batch2 = tuple(np.asarray(b, np.int64) for b in vbpr_ref.make_case(7, 5, 33, 65, seed=1).batch)
    names = ("Bi", "Gu", "Gi", "Tu", "E", "Bp")

    def model():
        m = mod.VBPRModel(case.F, case.Fd, lr, case.l_w, case.l_b, case.l_e, case.D, vbpr_ref.U, vbpr_ref.I, 42)
        for n in names:
            getattr(m, n).assign(getattr(case, n))
        return m

    def fed(b):
        u, i, j = b
        return (u, i, case.feat[i], j, case.feat[j])            # (user, pos, feature_pos, neg, feature_neg), :71

    def dense(g, like):
        if isinstance(g, tf.IndexedSlices):
            return torch.zeros(like.shape, dtype=g.values.dtype).index_add_(0, g.indices, g.values).numpy()
        return g.numpy()

    out = {n: getattr(case, n) for n in names}
    out.update({"feat": case.feat, "u": batch[0], "i": batch[1], "j": batch[2], "u2": batch2[0], "i2": batch2[1], "j2": batch2[2],
                "hyper": np.array([case.l_w, case.l_b, case.l_e, lr], np.float64)})
    m = model()
    m.optimizer = Recorder()
    out["loss"] = np.float64(float(m.train_step(fed(batch))))
    for n, g in zip(names, m.optimizer.grads):
        out["g" + n] = dense(g, getattr(case, n))
    m = model()
    out["loss_1"] = np.float64(float(m.train_step(fed(batch))))
    out["loss_2"] = np.float64(float(m.train_step(fed(batch2))))
    for n in names:
        out["after_" + n] = getattr(m, n).numpy()
    out["block"] = np.array([2, 6, 10, 40], np.int64)            # users [2, 6), items 10 .. 40 inclusive
    out["predict"] = m.predict_item_batch(2, 6, 10, 40, case.feat[10:41]).numpy()
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "vbpr_ref.npz"), **out)
    print("wrote", os.path.join(args.out, "vbpr_ref.npz"), {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
