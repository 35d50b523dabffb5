"""The TensorFlow half of the oracle against the reference's UNMODIFIED model files executed on the `tensorflow` stand-in of
oracle/tf_shim (torch-CPU autograd).  tests/golden/tfshim_*.npz are written by oracle/gen_golden_tfshim.py with
the generators -- injected weights, clause-hitting batches, file layout -- of oracle/gen_golden_tf.py; the checks are the ones the
real TensorFlow fixtures will go through (tests/helpers/tf_pins.py).

What this pins: the oracle's reading of the FILES (BPRMF_batch_model.py:47-88: which gathered tensors enter the L2 term, the / 10 on
the negative bias, the batch SUM; multi_vae_model.py:115-142: KL mean over batch and latent, the per-user log-likelihood mean;
neural_matrix_factorization_model.py:75-104: [mf ; mlp] in front of the head, Keras' loss wrapper; the GMF file).  What it does not:
TensorFlow's library behaviour -- the stand-in implements the same recalled clauses (oracle/tf_clauses.py).  (c) stays "parity
unpinned" until oracle/gen_golden_tf.py has run under tensorflow==2.3.2 (tests/test_tf_pins.py)."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.helpers import tf_pins

CHECKS = [("bprmf_batch", tf_pins.check_bprmf_batch), ("multivae", tf_pins.check_multivae), ("neumf", tf_pins.check_neumf),
          ("gmf", tf_pins.check_gmf)]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,check", CHECKS, ids=[c[0] for c in CHECKS])
def test_oracle_against_the_reference_files_on_the_stand_in(name, check):
    check(np.load(os.path.join(GOLDEN, f"tfshim_{name}.npz"), allow_pickle=False))


def test_a_flipped_clause_is_caught_on_these_fixtures():
    """Oracle and stand-in read the same switches at generation time; afterwards the fixtures are data: flipping a clause in the
    oracle alone makes the checks fail."""
    from oracle import tf_clauses
    d = np.load(os.path.join(GOLDEN, "tfshim_bprmf_batch.npz"), allow_pickle=False)
    n = np.load(os.path.join(GOLDEN, "tfshim_neumf.npz"), allow_pickle=False)
    for clause, data, check in (("adam_sparse_apply_moves_all_rows", d, tf_pins.check_bprmf_batch),
                                ("clip_gradient_inclusive_at_bound", d, tf_pins.check_bprmf_batch),
                                ("adam_one_minus_beta_in_fp32", d, tf_pins.check_bprmf_batch),
                                ("bce_adds_epsilon_inside_log", n, tf_pins.check_neumf),
                                ("adam_dense_uses_delta_form", n, None)):
        if check is None:
            continue
        old = tf_clauses.CLAUSES[clause]
        tf_clauses.CLAUSES[clause] = not old
        try:
            with pytest.raises(AssertionError):
                check(data)
        finally:
            tf_clauses.CLAUSES[clause] = old


def test_stand_in_never_reaches_the_product():
    """oracle/tf_shim is test infrastructure: nothing under elliot_amd/ or bench.py imports it (or tensorflow at all)."""
    for root, _, files in os.walk(os.path.join(REPO, "elliot_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "tf_shim" not in src and "import tensorflow" not in src, os.path.join(root, f)
    assert "tf_shim" not in open(os.path.join(REPO, "bench.py")).read()
