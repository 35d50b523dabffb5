"""GPU end-to-end: the nine fairness metrics through the plugin surface (RecMixin.train() / evaluate()) and the mini runner --
the device route, the dict route and `device_metrics: False` give the same numbers; the lists' scores travel to the evaluator only
when a *MADrating metric is configured; config_files/sample_fairness_amd.yml runs as it is."""
import math
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import yaml

from elliot_amd.synthetic import small_dataset
from tests.helpers import fair_ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_experiment(folder, metrics, n_users, n_items, seed):
    os.makedirs(folder)
    indptr, indices, _ = small_dataset(n_users, n_items, seed=seed)
    rs = np.random.RandomState(seed)
    users = np.repeat(np.arange(n_users), np.diff(indptr))
    with open(folder / "dataset.tsv", "w") as f:
        for u, i in zip(users, indices):
            f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")
    ilab, ulab = fair_ref.random_labels(n_items, 3, seed=seed + 1), fair_ref.random_labels(n_users, 2, seed=seed + 2)
    keep_i, keep_u = np.flatnonzero(ilab >= 0), np.flatnonzero(ulab >= 0)
    fair_ref.write_tsv(folder / "items.tsv", (keep_i + 1).tolist() + [n_items + 50], ilab[keep_i].tolist() + [1])      # one foreign id
    fair_ref.write_tsv(folder / "users.tsv", (keep_u + 1).tolist(), ulab[keep_u].tolist())
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": 10, "evaluation": {"cutoffs": [10, 5], "simple_metrics": ["nDCG"], "relevance_threshold": 3,
                                       "complex_metrics": fair_ref.complex_metrics("items.tsv", "users.tsv", metrics)},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/",
           "models": {"ItemKNN": {"meta": {"save_recs": False}, "neighbors": 20, "similarity": "cosine"}}}
    with open(folder / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    return exp


def same(a, b, what):
    """integers of the tables are compared in test_gpu_metrics_fair.py; here the values: within 1e-10, nan / inf alike"""
    assert list(a) == list(b) and len(a) > 1, (what, list(a), list(b))
    for m in a:
        x, y = a[m], b[m]
        if math.isnan(y) or math.isinf(y):
            assert (math.isnan(x) if math.isnan(y) else x == y), (what, m, x, y)
        else:
            assert abs(x - y) <= 1e-10 * abs(y), (what, m, x, y)


def fresh_model(runner, exp, folder, device_metrics=True, train=True):
    from elliot_amd.recommender import ItemKNN
    cfg = runner.build_config(exp, str(folder))
    cfg.device_metrics = device_metrics
    data = runner.load_data(exp, cfg, str(folder))
    model = ItemKNN(data=data, config=cfg, params=SimpleNamespace(meta=SimpleNamespace(verbose=False, save_recs=False), neighbors=20,
                                                                  similarity="cosine"))
    assert model._device_metrics() == device_metrics
    if train:
        model.train()
    return model


def test_device_route_equals_dict_route_with_all_nine(ctx, tmp_path):
    from elliot_amd import run as runner
    folder = tmp_path / "cfg"
    exp = write_experiment(folder, fair_ref.METRICS, 250, 200, seed=11)
    (name, res), = runner.run_experiment(str(folder / "exp.yml")).items()
    model = fresh_model(runner, exp, folder)
    device = model.get_results()
    host = model.evaluator.eval(model.get_recommendations(10))
    off = fresh_model(runner, exp, folder, device_metrics=False).get_results()
    for c in (10, 5):
        got = device[c]["test_results"]
        assert len(got) == 1 + 2 * 4 + 3 * 6 + 4 and list(got)[0] == "nDCG"
        assert "BiasDisparityBD_users:UG-1_items:IG-2" in got and "UserMADrating_UG" in got and "RSP_items:IG" in got
        same(res[c]["test_results"], got, f"runner@{c}")
        same(got, host[c]["test_results"], f"device vs dict route@{c}")
        same(off[c]["test_results"], host[c]["test_results"], f"device_metrics: False@{c}")
        assert device[c]["val_results"] == got
        assert all(math.isfinite(v) for v in got.values())


@pytest.mark.parametrize("rating", [True, False])
def test_scores_travel_only_for_the_rating_metrics(ctx, tmp_path, rating):
    from elliot_amd import run as runner
    from elliot_amd.evaluation.evaluator import EvalBlock
    folder = tmp_path / "cfg"
    metrics = [m for m in fair_ref.METRICS if rating or not m.endswith("MADrating")]
    exp = write_experiment(folder, metrics, 120, 90, seed=3)
    model = fresh_model(runner, exp, folder, train=False)
    assert model.evaluator.needs_scores == rating
    seen = {"recommend": [], "with_scores": 0, "blocks": 0}
    recommend, eval_device = model._model.recommend, model.evaluator.eval_device

    def counting_recommend(*args, **kwargs):
        idx, val = recommend(*args, **kwargs)
        seen["recommend"].append(val)
        return idx, val

    def counting_eval_device(ctx_, data, blocks):
        def watched():
            for b in blocks:
                seen["blocks"] += 1
                if isinstance(b, EvalBlock) and b.val_test is not None:
                    assert any(b.val_test is v for v in seen["recommend"])
                    seen["with_scores"] += 1
                else:
                    assert len(b) == 3
                yield b
        return eval_device(ctx_, data, watched())

    model._model.recommend, model.evaluator.eval_device = counting_recommend, counting_eval_device
    model.train()
    assert seen["blocks"] >= 1 and len(seen["recommend"]) == seen["blocks"]
    assert seen["with_scores"] == (seen["blocks"] if rating else 0)


def test_the_sample_configuration_runs(ctx, tmp_path):
    from elliot_amd.run import run_experiment
    shutil.copytree(os.path.join(REPO, "config_files", "attribute_sample"), tmp_path / "config_files" / "attribute_sample")
    with open(os.path.join(REPO, "config_files", "sample_fairness_amd.yml")) as fh:
        cfg = yaml.safe_load(fh)
    for key in ("path_output_rec_result", "path_output_rec_weight", "path_output_rec_performance"):
        cfg["experiment"][key] = str(tmp_path / "out" / key)
    with open(tmp_path / "config_files" / "sample_fairness_amd.yml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    (name, res), = run_experiment(str(tmp_path / "config_files" / "sample_fairness_amd.yml")).items()
    for c in (10, 5):
        got = res[c]["test_results"]
        assert len(got) == 1 + 2 * 4 + 3 * 6 + 4
        assert "RSP_items:ItemPopularity" in got and "BiasDisparityBD_users:UserActivity-1_items:ItemPopularity-2" in got
        assert all(math.isfinite(v) for v in got.values())
