"""Host: the factoring el_fism.hip rests on.  The float64 restatement of the reference (tests/helpers/fism_ref.py: padded history
matrix, [B, L, F] gathers, swapped loss arguments, autograd) gives the gradients that the factored formulas of include/elliot_hip.h
(el_fism_grads), evaluated in numpy float64, give -- on 7 users and 9 items with padded slots, a repeated user, a repeated item and
item 0 in a history -- to 1e-12, for both loss kinds and with and without the padded slots.  And ops.fism_history_index is the
exact transpose of the histories, users ascending in every list."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import fism_ref


def small_case():
    rs = np.random.RandomState(5)
    hist = [np.array(h) for h in ([3, 0, 5], [1], [8, 2, 4, 6, 0], [7, 3], [2], [5, 6, 1, 8], [4, 0])]
    lens = np.array([len(h) for h in hist])
    t = lambda lo, hi, *s: rs.uniform(lo, hi, s).astype(np.float32)                       # noqa: E731
    batch = (np.array([2, 0, 2, 6, 3, 2, 1], np.int32), np.array([4, 7, 1, 7, 0, 8, 1], np.int32),
             np.array([5, 0, 0.5, 1, 0, 3, 0], np.float32))
    return SimpleNamespace(U=7, I=9, F=4, L=5, hist=hist, lens=lens, coef=np.power(lens.astype(np.float32), np.float32(-0.5)),
                           Gi=t(-0.5, 0.5, 9, 4), Gj=t(-0.5, 0.5, 9, 4), Bu=t(-0.2, 0.2, 7), Bi=t(-0.2, 0.2, 9), beta=0.01, lam=0.02,
                           gamma=0.03, batch=batch)


@pytest.mark.parametrize("loss", ["reference", "bce"])
@pytest.mark.parametrize("pad", [True, False])
def test_autograd_of_the_restatement_equals_the_factored_formulas(loss, pad):
    case = small_case()
    want = fism_ref.Model(case, torch.float64, pad=pad, loss=loss).gradients(case.batch, chunk=3)[1:]
    got = fism_ref.factored(case, case.batch, case.L if pad else 0, loss)
    for n, a, b in zip(fism_ref.NAMES, got, want):
        assert np.abs(a - b.numpy()).max() < 1e-12, n
    assert np.abs(got[0]).max() > 1e-3 and (case.batch[0] == 2).sum() == 3 and 0 in case.hist[2]


def test_history_index_is_the_exact_transpose():
    from elliot_amd import ops
    case = small_case()
    indptr = np.concatenate([[0], np.cumsum(case.lens)])
    hp, hi, tp, ti = ops.fism_history_index(indptr, np.concatenate(case.hist), case.I)
    assert np.array_equal(hi, np.concatenate(case.hist)) and tp[-1] == hp[-1]
    for k in range(case.I):
        assert ti[tp[k]:tp[k + 1]].tolist() == [u for u in range(case.U) if k in case.hist[u]]
