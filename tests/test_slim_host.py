"""Slim's host surface: the plugin is exported where the runner and an unmodified Elliot look for it, and the C ABI binds the four
entry points the model is built from.  No GPU."""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plugin_is_exported():
    from elliot_amd import recommender
    from elliot_amd.recommender import Slim
    assert "Slim" in recommender.__all__
    assert Slim.__module__ == "elliot_amd.recommender.latent_factor_models.Slim.slim"
    for hook in ("train", "name", "get_recommendations", "restore_weights"):
        assert hasattr(Slim, hook), hook


def test_external_entry_point_resolves():
    """elliot/run.py loads external/__init__.py by path as the package `external` and resolves the class with getattr."""
    spec = importlib.util.spec_from_file_location("external", os.path.join(REPO, "elliot_amd", "external", "__init__.py"))
    external = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(external)
    from elliot_amd.recommender import Slim
    assert external.Slim is Slim
    assert "external.Slim" in external.__doc__


def test_model_class_surface():
    from elliot_amd.recommender.latent_factor_models.Slim.slim_model import SlimModel
    for hook in ("initialize", "recommend", "w_csr", "get_model_state", "set_model_state", "save_weights", "load_weights"):
        assert callable(getattr(SlimModel, hook)), hook


def test_prototypes_are_bound():
    from elliot_amd import _lib, ops
    for name in ("el_slim_order", "el_slim_ws_bytes", "el_slim_fit", "el_slim_w"):
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.load(), name), name
    for name in ("slim_order", "slim_fit", "slim_w", "slim_build", "slim_csc"):
        assert callable(getattr(ops, name)), name
    assert _lib.load().el_abi_version() == 8                      # entry points are only added


def test_workspace_sizes():
    """Host-only entry point: 0 for empty problems; the LDS placement needs a norm per column and target only, the global
    placement a residual and a weight vector per target on top; el_slim_w's size does not depend on the users."""
    from elliot_amd import _lib
    lib = _lib.load()
    assert lib.el_slim_ws_bytes(0, 10, 1, 10) == 0 and lib.el_slim_ws_bytes(100, 100, 1, 0) == 0
    lds1, lds9 = lib.el_slim_ws_bytes(6040, 3706, 1, 10), lib.el_slim_ws_bytes(6040, 3706, 9, 10)
    assert 0 < lds1 < lds9 and (lds9 - lds1) // 8 < 2 * 3706 * 4
    glob1, glob9 = lib.el_slim_ws_bytes(138493, 26744, 1, 10), lib.el_slim_ws_bytes(138493, 26744, 9, 10)
    assert (glob9 - glob1) // 8 >= (138493 + 2 * 26744) * 4
    assert lib.el_slim_ws_bytes(37000, 3706, 2, 10) - lib.el_slim_ws_bytes(37000, 3706, 1, 10) < 4 * 37000      # still LDS
    assert lib.el_slim_ws_bytes(38000, 3706, 2, 10) - lib.el_slim_ws_bytes(38000, 3706, 1, 10) >= 4 * 38000     # the workspace
    assert lib.el_slim_ws_bytes(5, 3706, 0, 10) == lib.el_slim_ws_bytes(10 ** 6, 3706, 0, 10) >= 3706 * 10 * 8


def test_penalties_and_seed_state_are_sklearns():
    from elliot_amd import ops
    from tests.helpers import slim_ref
    for alpha, l1_ratio, U in ((0.001, 0.001, 300), (0.01, 0.1, 6040), (1.0, 0.01, 138493)):
        l1, l2 = ops.slim_penalties(alpha, l1_ratio, U)
        r1, r2 = slim_ref.penalties(alpha, l1_ratio, U)
        assert np.float32(l1) == r1 and np.float32(l2) == r2
    assert ops.slim_seed_state(42) == slim_ref.seed_state(42) == int(np.random.RandomState(42).randint(0, 2147483647))


def test_sample_config_names_the_model():
    import yaml
    with open(os.path.join(REPO, "config_files", "sample_slim_amd.yml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg["experiment"]["models"]) == {"Slim"}
    assert set(cfg["experiment"]["models"]["Slim"]) == {"meta", "l1_ratio", "alpha", "neighborhood", "exclusion"}
