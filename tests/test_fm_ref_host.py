"""Host: the restatement the FM GPU tests rest on (tests/helpers/fm_ref.py) and the index structures the plugin builds.

The factored form the kernels use (s_i, q_i, l_i) equals the one-hot form of the reference in float64 to 1e-12 on the case
tables; the feature-major copy of the attribute matrix is the exact transpose of the item-major one."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from tests.helpers import fm_ref


@pytest.mark.parametrize("nF,kind", [(70, "mixed"), (70, "every"), (1, "mixed"), (0, "mixed")])
def test_factored_form_equals_the_one_hot_form(nF, kind):
    case = fm_ref.make_case(10, 65, nF, kind)
    m = fm_ref.Model(case, torch.float64)
    uu, ii = np.meshgrid(np.arange(case.U), np.arange(case.I), indexing="ij")
    a, b = m.predict(uu.reshape(-1), ii.reshape(-1)).numpy(), m.factored(uu.reshape(-1), ii.reshape(-1)).numpy()
    assert np.abs(a - b).max() <= 1e-12
    if nF == 70:                                                # what make_case promises
        f = case.feats
        assert (f[0] == [67] if kind == "every" else f[0] == []) and len(f[2]) >= 40 and f[3] == f[4] and len(f[3]) >= 3
        assert all(68 not in f[i] for i in case.batch[1]) and 68 in f[case.I - 1]
        assert (case.batch[0][0], case.batch[1][0]) == (case.batch[0][1], case.batch[1][1])


@pytest.mark.parametrize("nF,kind", [(70, "every"), (1, "mixed"), (0, "mixed")])
def test_feature_major_index_is_the_exact_transpose(nF, kind):
    case = fm_ref.make_case(3, 65, nF, kind)
    ap, ai, tp, ti = ops.fm_attribute_index([f + f[:1] for f in case.feats], nF)      # (a repeated id counts once)
    A = sp.csr_matrix((np.ones(len(ai)), ai, ap), shape=(case.I, max(nF, 1)))
    T = sp.csr_matrix((np.ones(len(ti)), ti, tp), shape=(nF, case.I)) if nF else None
    assert A.nnz == sum(len(f) for f in case.feats) and all(ai[ap[i]:ap[i + 1]].tolist() == case.feats[i] for i in range(case.I))
    if nF:
        assert (A[:, :nF].T.tocsr() != T).nnz == 0 and all(np.all(np.diff(ti[tp[f]:tp[f + 1]]) > 0) for f in range(nF))
    else:
        assert len(ti) == 0 and tp.tolist() == [0]
