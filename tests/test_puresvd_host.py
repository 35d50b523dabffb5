"""PureSVD's host surface: parameters and `name`, the shape rules of the method, the refusals that need no device, the checkpoint
(also one written with the reference's keys), registration and the C ABI.  No GPU: the plugin is built on a stand-in context whose
buffers live in host memory; nothing here launches a kernel."""
import importlib.util
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import psvd_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UOFF, IOFF = 1000, 5000


@pytest.fixture
def host_ctx(monkeypatch):
    """ops.get_context -> a context without a library handle, on the CPU device, with 1 GiB 'free'."""
    from elliot_amd import ops
    ctx = SimpleNamespace(device=torch.device("cpu"), lib=None, handle=None)
    monkeypatch.setattr(ops, "get_context", lambda device=0: ctx)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 30, 1 << 30))
    return ctx


def params(**kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    return SimpleNamespace(meta=meta, **kw)


def dataset(tmp_path, U=60, I=40, seed=3):
    from elliot_amd.dataset.dataset import DataSet, default_config
    cfg = default_config(top_k=10, cutoffs=[10, 5], simple_metrics=["nDCG", "Recall"], out_dir=str(tmp_path))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    rs = np.random.RandomState(seed)
    dense = rs.rand(U, I) < 0.2
    dense[np.arange(U), rs.randint(0, I, U)] = True
    dense[rs.randint(0, U, I), np.arange(I)] = True
    u, i = np.nonzero(dense)
    te_u = np.arange(U)
    te_i = np.array([rs.choice(np.flatnonzero(~dense[x])) for x in range(U)])
    return DataSet(cfg, (u + UOFF, i + IOFF, np.ones(u.shape[0])), (te_u + UOFF, te_i + IOFF, np.ones(U))), cfg


def test_plugin_is_exported():
    from elliot_amd import recommender
    from elliot_amd.recommender import PureSVD
    assert "PureSVD" in recommender.__all__
    assert PureSVD.__module__ == "elliot_amd.recommender.latent_factor_models.PureSVD.pure_svd"
    for hook in ("train", "name", "predict", "get_recommendations", "restore_weights"):
        assert hasattr(PureSVD, hook), hook


def test_external_entry_point_resolves():
    spec = importlib.util.spec_from_file_location("external", os.path.join(REPO, "elliot_amd", "external", "__init__.py"))
    external = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(external)
    from elliot_amd.recommender import PureSVD
    assert external.PureSVD is PureSVD
    assert "external.PureSVD" in external.__doc__


def test_prototypes_are_bound():
    from elliot_amd import _lib, ops
    for name in ("el_spmm_csr_f64_ws_bytes", "el_spmm_csr_f64", "el_gram_f64_slots", "el_gram_f64_ws_bytes", "el_gram_f64",
                 "el_psvd_orth_ws_bytes", "el_psvd_orth", "el_psvd_project", "el_psvd_signs_ws_bytes", "el_psvd_signs"):
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.load(), name), name
    for name in ("spmm_csr_f64", "gram_f64", "psvd_orth", "psvd_project", "psvd_signs", "PureSvdDeviceState"):
        assert callable(getattr(ops, name)), name
    assert _lib.EL_PSVD_MAX_R == 256
    assert _lib.load().el_abi_version() == 8                      # entry points are only added


def test_workspace_sizes():
    """Host-only entry points: the Gram's slot count depends on the rows only and is capped; sizes are 0 for empty problems."""
    from elliot_amd import _lib
    lib = _lib.load()
    assert [lib.el_gram_f64_slots(n) for n in (0, 1, 1024, 1025, 6040, 10 ** 6)] == [1, 1, 1, 2, 6, 256]
    assert lib.el_gram_f64_ws_bytes(6040, 60) >= 6 * 60 * 60 * 8
    assert lib.el_psvd_orth_ws_bytes(6040, 60) >= lib.el_gram_f64_ws_bytes(6040, 60) + 3 * 60 * 60 * 8
    assert lib.el_spmm_csr_f64_ws_bytes(0, 60) == 0 and lib.el_spmm_csr_f64_ws_bytes(7, 60) >= 7 * 60 * 8
    assert lib.el_psvd_signs_ws_bytes(1000, 50) >= 2 * 50 * 8 and lib.el_psvd_signs_ws_bytes(0, 50) == 0


def test_orientation_and_iteration_rule():
    """sklearn's defaults: n_iter = 7 below a tenth of the smaller side, else 4; the method runs on A^T when U < I."""
    from elliot_amd import ops
    assert ops.psvd_plan(300, 200, 10) == (20, 7, False)
    assert ops.psvd_plan(200, 320, 10) == (20, 7, True)
    assert ops.psvd_plan(150, 120, 16) == (26, 4, False)
    assert ops.psvd_plan(150, 120, 12) == (22, 4, False)           # 12 < 12.0 is false
    assert ops.psvd_plan(150, 120, 11) == (21, 7, False)
    assert ops.psvd_plan(500, 500, 49) == (59, 7, False)           # a square matrix is not transposed
    assert ops.psvd_plan(6040, 3706, 246) == (256, 7, False)
    for U, I, f in ((300, 200, 10), (200, 320, 10), (150, 120, 16), (600, 900, 100)):
        assert ops.psvd_plan(U, I, f) == psvd_ref.plan(U, I, f)


def test_start_matrix_is_the_references_draw():
    from elliot_amd import ops
    Q = ops.psvd_start_matrix(37, 13, 42)
    ref = np.random.RandomState(42).normal(size=(37, 13))
    assert Q.dtype == np.float64 and np.array_equal(Q, ref.astype(np.float32).astype(np.float64)) and not np.array_equal(Q, ref)
    assert np.array_equal(Q, psvd_ref.start_matrix(37, 13, 42))
    assert not np.array_equal(Q, ops.psvd_start_matrix(37, 13, 7))


def test_small_svd_host_step():
    """eigh of Z^T Z gives the singular values and the matrices that turn the two bases into the tables, for both orientations."""
    from elliot_amd import ops
    rs = np.random.RandomState(0)
    Z = rs.normal(size=(50, 12)) * np.linspace(5, 1, 12)[None, :]
    s, wu, wi = ops.psvd_small_svd(Z.T @ Z, 4, False)
    assert np.allclose(s, np.linalg.svd(Z, compute_uv=False)[:4], rtol=1e-12) and np.array_equal(wu, wi) and wu.shape == (12, 4)
    s2, wu2, wi2 = ops.psvd_small_svd(Z.T @ Z, 4, True)
    assert np.array_equal(s2, s) and np.allclose(wu2 * s, wu) and np.allclose(wi2 / s, wu)


@pytest.mark.parametrize("factors, pattern", [(0, "must be an integer >= 1"), (-3, "must be an integer >= 1"),
                                              (2.5, "must be an integer >= 1"), (247, "at most 256"), (31, "exceeds min")])
def test_refusals_of_the_shape_rules(factors, pattern):
    from elliot_amd import ops
    U, I = (10 ** 4, 10 ** 4) if factors == 247 else (60, 40)
    with pytest.raises(ValueError, match=pattern):
        ops.psvd_plan(U, I, factors)


def test_refusal_of_a_set_orthonormalisation_status():
    from elliot_amd import ops
    ops.psvd_check_rank(0x7fffffff, 42)
    with pytest.raises(ValueError, match=r"column 39 of 42.*rank"):
        ops.psvd_check_rank(39, 42)


def test_plugin_refuses_before_anything_is_built(host_ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = dataset(tmp_path)
    for factors, pattern in ((0, ">= 1"), (247, "at most 256"), (31, "exceeds min")):
        with pytest.raises(ValueError, match=pattern):
            PureSVD(data=data, config=cfg, params=params(factors=factors))


def test_memory_need_is_refused_with_the_bytes(host_ctx, tmp_path, monkeypatch):
    from elliot_amd import ops
    from elliot_amd.recommender import PureSVD
    data, cfg = dataset(tmp_path)
    need = ops.psvd_memory_need(60, 40, data.sp_i_train.nnz, 10)
    assert need >= 8 * 20 * 100 + 8 * data.sp_i_train.nnz
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need - 1, 1 << 30))
    with pytest.raises(ValueError, match=f"{need} bytes"):
        PureSVD(data=data, config=cfg, params=params(factors=10))


def test_parameters_and_name(host_ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = dataset(tmp_path)
    model = PureSVD(data=data, config=cfg, params=params())
    assert model._factors == 10 and model._seed == 42 and model.name == "PureSVD_factors=10"
    assert model._params_list == [("_factors", "factors", "factors", 10, None, None)]
    model = PureSVD(data=data, config=cfg, params=params(factors=20, seed=7))
    assert model.name == "PureSVD_factors=20" and model._model.random_seed == 7
    st = model._model.state
    assert (st.U, st.I, st.R, st.n_iter, st.transposed) == (60, 40, 30, 4, False)
    assert os.path.isdir(os.path.join(cfg.path_output_rec_weight, model.name))


def test_checkpoint_round_trip_and_reference_keys(host_ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = dataset(tmp_path)
    model = PureSVD(data=data, config=cfg, params=params(factors=5))
    rs = np.random.RandomState(1)
    # what the reference's save_weights writes: its own keys, float32 tables
    ref_state = {"user_vec": rs.normal(size=(60, 5)).astype(np.float32), "item_vec": rs.normal(size=(40, 5)).astype(np.float32)}
    path = tmp_path / "reference-weights"
    with open(path, "wb") as f:
        pickle.dump(ref_state, f)
    model._model.load_weights(str(path))
    state = model._model.get_model_state()
    assert set(state) == {"user_vec", "item_vec"}
    assert np.array_equal(state["user_vec"], ref_state["user_vec"]) and np.array_equal(state["item_vec"], ref_state["item_vec"])
    u, i = 17, 23
    assert model.predict(u + UOFF, i + IOFF) == ref_state["user_vec"][data.public_users[u + UOFF]].dot(
        ref_state["item_vec"][data.public_items[i + IOFF]])
    out = tmp_path / "again"
    model._model.save_weights(str(out))
    again = PureSVD(data=data, config=cfg, params=params(factors=5))
    again._model.load_weights(str(out))
    assert np.array_equal(again._model.get_model_state()["item_vec"], ref_state["item_vec"])
    with pytest.raises(ValueError, match="shapes"):
        again._model.set_model_state({"user_vec": ref_state["user_vec"][:10], "item_vec": ref_state["item_vec"]})


def test_sample_config_names_the_model():
    import yaml
    with open(os.path.join(REPO, "config_files", "sample_puresvd_amd.yml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg["experiment"]["models"]) == {"PureSVD"}
    assert set(cfg["experiment"]["models"]["PureSVD"]) == {"meta", "factors", "seed"}


def test_spmm_order_restatement_is_a_plain_product():
    """The documented order of el_spmm_csr_f64 (tests/helpers/psvd_ref.py::spmm_ordered) is a product: equal to scipy's up to rounding,
    and equal bit for bit where every sum is exact (small integers)."""
    import scipy.sparse as sp
    rs = np.random.RandomState(2)
    A = sp.random(30, 25, density=0.4, random_state=rs, format="csr", dtype=np.float32)
    A.data[:] = rs.randint(1, 4, A.nnz)
    X = rs.randint(-8, 9, size=(25, 7)).astype(np.float64)
    for piece in (4, 1000):
        assert np.array_equal(psvd_ref.spmm_ordered(A.indptr, A.indices, A.data, X, piece), A.astype(np.float64) @ X)
    assert np.array_equal(psvd_ref.spmm_ordered(A.indptr, A.indices, None, X, 4), (A != 0).astype(np.float64) @ X)
