"""RP3beta's host surface: the plugin is exported where the runner and an unmodified Elliot look for it, and the C ABI binds the
four entry points the model is built from.  No GPU."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plugin_is_exported():
    from elliot_amd import recommender
    from elliot_amd.recommender import RP3beta
    assert "RP3beta" in recommender.__all__
    assert RP3beta.__module__ == "elliot_amd.recommender.graph_based.RP3beta.rp3beta"
    for hook in ("train", "name", "get_recommendations", "restore_weights"):
        assert hasattr(RP3beta, hook), hook


def test_external_entry_point_resolves():
    """elliot/run.py loads external/__init__.py by path as the package `external` and resolves the class with getattr."""
    spec = importlib.util.spec_from_file_location("external", os.path.join(REPO, "elliot_amd", "external", "__init__.py"))
    external = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(external)
    from elliot_amd.recommender import RP3beta
    assert external.RP3beta is RP3beta
    assert "external.RP3beta" in external.__doc__


def test_mini_runner_resolves_both_keys():
    from elliot_amd import recommender as rec
    for key in ("RP3beta", "external.RP3beta"):
        assert getattr(rec, key.split(".")[-1], None) is rec.RP3beta


def test_model_class_surface():
    from elliot_amd.recommender.graph_based.RP3beta.rp3beta_model import RP3betaModel
    for hook in ("initialize", "recommend", "w_csr", "get_model_state", "set_model_state", "save_weights", "load_weights"):
        assert callable(getattr(RP3betaModel, hook)), hook


def test_prototypes_are_bound():
    from elliot_amd import _lib, ops
    for name in ("el_csr_row_l1", "el_rp3_ws_bytes", "el_rp3_rows", "el_rp3_cut"):
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.load(), name), name
    for name in ("csr_row_l1", "rp3_operands", "rp3_rows", "rp3_cut", "rp3_build"):
        assert callable(getattr(ops, name)), name


def test_workspace_sizes():
    """Host-only entry point: 0 for empty problems, the row workspace grows with the rows of one call, the cut's does not."""
    from elliot_amd import _lib
    lib = _lib.load()
    assert lib.el_rp3_ws_bytes(0, 10, 1) == 0 and lib.el_rp3_ws_bytes(100, 0, 1) == 0
    assert 0 < lib.el_rp3_ws_bytes(40000, 50, 1) < lib.el_rp3_ws_bytes(40000, 50, 1000)
    assert lib.el_rp3_ws_bytes(40000, 50, 0) >= 40000 * 50 * 4 * 5
    assert lib.el_rp3_ws_bytes(120, -1, 0) == 0


def test_sample_config_names_the_model():
    import yaml
    with open(os.path.join(REPO, "config_files", "sample_rp3beta_amd.yml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg["experiment"]["models"]) == {"RP3beta"}
    assert set(cfg["experiment"]["models"]["RP3beta"]) == {"meta", "neighborhood", "alpha", "beta", "normalize_similarity"}
