"""GPU end-to-end: the metric list of config_files/sample_beyond_accuracy_amd.yml (and the other beyond-accuracy names) through
the mini runner and the plugin surface -- device route, dict route and `device_metrics: False` give the same numbers."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import yaml

from elliot_amd import ops
from elliot_amd.synthetic import small_dataset

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ["nDCG", "Precision"] + list(ops.BEYOND_METRIC_NAMES)


def sample_metrics():
    with open(os.path.join(REPO, "config_files", "sample_beyond_accuracy_amd.yml")) as f:
        return yaml.safe_load(f)["experiment"]["evaluation"]["simple_metrics"]


def write_experiment(folder, metrics, n_users, n_items, seed, **extra):
    os.makedirs(folder)
    indptr, indices, _ = small_dataset(n_users, n_items, seed=seed)
    rs = np.random.RandomState(seed)
    users = np.repeat(np.arange(n_users), np.diff(indptr))
    with open(folder / "dataset.tsv", "w") as f:
        for u, i in zip(users, indices):
            f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": 10, "evaluation": {"cutoffs": [10, 5], "simple_metrics": list(metrics), "relevance_threshold": 3},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/",
           "models": {"ItemKNN": {"meta": {"save_recs": False}, "neighbors": 20, "similarity": "cosine"}}}
    exp.update(extra)
    with open(folder / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    return exp


def same(a, b, names, what):
    assert list(a) == list(names) == list(b), (what, list(a), list(b))
    for m in names:
        x, y = a[m], b[m]
        if isinstance(y, int):
            assert isinstance(x, int) and x == y, (what, m, x, y)
        elif math.isnan(y):                                  # a head / tail ratio without a denominator, on both routes
            assert math.isnan(x), (what, m, x, y)
        else:
            assert abs(x - y) <= 1e-11 * abs(y), (what, m, x, y)


def fresh_model(runner, exp, folder, device_metrics=True):
    from elliot_amd.recommender import ItemKNN
    cfg = runner.build_config(exp, str(folder))
    cfg.device_metrics = device_metrics
    data = runner.load_data(exp, cfg, str(folder))
    model = ItemKNN(data=data, config=cfg, params=SimpleNamespace(meta=SimpleNamespace(verbose=False, save_recs=False), neighbors=20,
                                                                  similarity="cosine"))
    assert model._device_metrics() == device_metrics
    model.train()
    return model


@pytest.mark.parametrize("which", ["sample", "all"])
def test_runner_device_route_equals_dict_route(ctx, tmp_path, which):
    from elliot_amd import run as runner
    metrics = sample_metrics() if which == "sample" else ALL
    assert which == "all" or metrics == ["nDCG", "Precision", "ItemCoverage", "EPC", "Gini"]
    folder = tmp_path / "cfg"
    exp = write_experiment(folder, metrics, 250, 200, seed=11)
    (name, res), = runner.run_experiment(str(folder / "exp.yml")).items()
    model = fresh_model(runner, exp, folder)
    device = model.get_results()
    host = model.evaluator.eval(model.get_recommendations(10))
    off = fresh_model(runner, exp, folder, device_metrics=False).get_results()
    for c in (10, 5):
        same(res[c]["test_results"], device[c]["test_results"], metrics, f"runner@{c}")
        same(device[c]["test_results"], host[c]["test_results"], metrics, f"device vs dict route@{c}")
        same(off[c]["test_results"], host[c]["test_results"], metrics, f"device_metrics: False@{c}")
        assert device[c]["val_results"] == device[c]["test_results"]
    assert 0 < device[10]["test_results"]["ItemCoverage"] <= model._data.num_items
    assert 0.0 < device[10]["test_results"]["Gini"] < 1.0


def test_validation_split_uses_the_validation_candidates(ctx, tmp_path):
    from elliot_amd import run as runner
    folder = tmp_path / "cfg"
    exp = write_experiment(folder, ALL, 220, 260, seed=5, negative_sampling={"strategy": "random", "num_items": 40})
    exp["splitting"]["validation_splitting"] = {"strategy": "random_subsampling", "test_ratio": 0.2}
    with open(folder / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    model = fresh_model(runner, exp, folder)
    assert hasattr(model._data, "val_dict")
    device = model.get_results()
    host = model.evaluator.eval(model.get_recommendations(10))
    for c in (10, 5):
        same(device[c]["test_results"], host[c]["test_results"], ALL, f"test@{c}")
        same(device[c]["val_results"], host[c]["val_results"], ALL, f"val@{c}")
        assert device[c]["val_results"] != device[c]["test_results"]
