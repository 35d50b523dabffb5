"""GPU end-to-end: the ItemKNN / UserKNN plugins through the mini runner and the plugin surface (item_knn.py / user_knn.py)."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.synthetic import small_dataset
from tests.helpers import knn_ref

pytestmark = pytest.mark.gpu

REF_NAME = "ItemKNN_nn=50_sim=cosine_imp=standard_bin=False_shrink=0_norm=True_asymalpha=_tvalpha=_tvbeta=_rweights="


def make_data(tmp_path):
    indptr, indices, _ = small_dataset(260, 200, seed=6)
    rs = np.random.RandomState(4)
    U = indptr.shape[0] - 1
    users = np.repeat(np.arange(U), np.diff(indptr))
    ratings = rs.randint(1, 6, indices.shape[0]).astype(float)
    flag = np.zeros(indices.shape[0], bool)
    for u in range(U):
        a, b = indptr[u], indptr[u + 1]
        n_te = (b - a) // 5
        if n_te:
            flag[a + rs.choice(b - a, n_te, replace=False)] = True
    cfg = default_config(top_k=10, cutoffs=[10, 5], simple_metrics=["nDCG", "Recall"], out_dir=str(tmp_path))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    tr = (users[~flag] + 1000, indices[~flag] + 5000, ratings[~flag])
    te = (users[flag] + 1000, indices[flag] + 5000, ratings[flag])
    return DataSet(cfg, tr, te), cfg


def params(**kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    return SimpleNamespace(meta=meta, **kw)


def write_tsv(path, n_users, n_items, seed):
    indptr, indices, _ = small_dataset(n_users, n_items, seed=seed)
    rs = np.random.RandomState(seed)
    users = np.repeat(np.arange(n_users), np.diff(indptr))
    with open(path, "w") as f:
        for u, i in zip(users, indices):
            f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")


def test_mini_runner_item_and_user_knn(ctx, tmp_path):
    import yaml
    from elliot_amd.run import run_experiment
    write_tsv(tmp_path / "dataset.tsv", 250, 200, seed=11)
    cfg = {"experiment": {
        "dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
        "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
        "top_k": 10, "evaluation": {"simple_metrics": ["nDCG"]},
        "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/",
        "path_output_rec_performance": "out/perf/",
        "models": {"ItemKNN": {"meta": {"save_recs": True}, "neighbors": 50, "similarity": "cosine"},
                   "external.UserKNN": {"meta": {"save_recs": True}, "neighbors": 30, "similarity": "dot", "implicit": True}}}}
    with open(tmp_path / "exp.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    res = run_experiment(str(tmp_path / "exp.yml"))
    assert set(res) == {REF_NAME, "UserKNN_nn=30_sim=dot_imp=standard_bin=True_shrink=0_norm=True_asymalpha=_tvalpha=_tvbeta=_rweights="}
    for r in res.values():
        assert 0.0 <= r[10]["test_results"]["nDCG"] <= 1.0
    recs = sorted(os.listdir(tmp_path / "out" / "recs"))
    assert recs == sorted(f"{n}.tsv" for n in res)
    assert os.path.getsize(tmp_path / "out" / "recs" / f"{REF_NAME}.tsv") > 0


@pytest.mark.parametrize("model_name", ["ItemKNN", "UserKNN"])
def test_dict_route_equals_device_route(ctx, tmp_path, model_name):
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    model = getattr(rec, model_name)(data=data, config=cfg, params=params(neighbors=25, similarity="cosine"))
    assert model._device_metrics()
    model.train()
    device = model.get_results()[10]["test_results"]["nDCG"]
    host = model.evaluator.eval(model.get_recommendations(10))[10]["test_results"]["nDCG"]
    assert 0.0 < device <= 1.0 and abs(device - host) < 1e-9


def test_lists_equal_restatement(ctx, tmp_path):
    """The plugin's lists are the restatement's top-k over R.dot(W) in public ids."""
    from elliot_amd.recommender import ItemKNN
    data, cfg = make_data(tmp_path)
    model = ItemKNN(data=data, config=cfg, params=params(neighbors=25, similarity="cosine"))
    model.train()
    _, recs = model.get_recommendations(10)
    R = data.sp_i_train_ratings
    W = knn_ref.build_w(R, "item", 25, "cosine")
    users = np.arange(data.num_users)
    idx, val = knn_ref.topk(knn_ref.scores(R, W, "item"), users, 10, excl=(R.indptr, R.indices))
    for u in users:
        exp = [(data.private_items[i], np.float32(v)) for i, v in zip(idx[u], val[u]) if i >= 0]
        got = recs[data.private_users[u]]
        assert [(i, np.float32(v)) for i, v in got] == exp, u


def test_sampled_negatives(ctx, tmp_path):
    import yaml
    from elliot_amd import run as runner
    os.makedirs(tmp_path / "cfg")
    write_tsv(tmp_path / "cfg" / "dataset.tsv", 180, 260, seed=5)
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "negative_sampling": {"strategy": "random", "num_items": 40},
           "top_k": 10, "evaluation": {"simple_metrics": ["nDCG", "HR"]},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/",
           "models": {"UserKNN": {"meta": {"save_recs": False}, "neighbors": 20, "similarity": "cosine"},
                      "ItemKNN": {"meta": {"save_recs": False}, "neighbors": 20, "similarity": "dot"}}}
    with open(tmp_path / "cfg" / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    res = runner.run_experiment(str(tmp_path / "cfg" / "exp.yml"))
    assert len(res) == 2
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["HR"] <= 1.0
    cfg = runner.build_config(exp, str(tmp_path / "cfg"))
    data = runner.load_data(exp, cfg, str(tmp_path / "cfg"))
    from elliot_amd.recommender import UserKNN
    model = UserKNN(data=data, config=cfg, params=params(neighbors=20, similarity="cosine"))
    model.train()
    _, recs = model.get_recommendations(10)
    for u, lst in recs.items():
        assert not ({i for i, _ in lst} & set(data.train_dict[u])), u
    dict_route = model.evaluator.eval(model.get_recommendations(10))
    assert abs(dict_route[10]["test_results"]["nDCG"] - model.get_results()[10]["test_results"]["nDCG"]) < 1e-9


def test_name_matches_reference_format(ctx, tmp_path):
    from elliot_amd.recommender import ItemKNN, UserKNN
    data, cfg = make_data(tmp_path)
    assert ItemKNN(data=data, config=cfg, params=params(neighbors=50, similarity="cosine")).name == REF_NAME
    u = UserKNN(data=data, config=cfg, params=params(neighbors=40, similarity="dot", shrink=5))
    assert u.name == "UserKNN_nn=40_sim=dot_imp=standard_bin=False_shrink=5_norm=True_asymalpha=_tvalpha=_tvbeta=_rweights="


def test_options_refused(ctx, tmp_path):
    from elliot_amd.recommender import ItemKNN, UserKNN
    data, cfg = make_data(tmp_path)
    with pytest.raises(NotImplementedError, match="aiolli"):
        ItemKNN(data=data, config=cfg, params=params(implementation="aiolli"))
    with pytest.raises(ValueError, match="cosine"):
        UserKNN(data=data, config=cfg, params=params(similarity="jaccard"))


@pytest.mark.parametrize("model_name", ["ItemKNN", "UserKNN"])
def test_save_restore_round_trip(ctx, tmp_path, model_name):
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    cls = getattr(rec, model_name)
    model = cls(data=data, config=cfg, params=params(neighbors=15, similarity="cosine", meta={"save_weights": True}))
    model.train()
    assert os.path.exists(model._saving_filepath)
    before = model.get_recommendations(10)[1]
    again = cls(data=data, config=cfg, params=params(neighbors=15, similarity="cosine", meta={"restore": True}))
    again.train()
    assert again.get_recommendations(10)[1] == before
    assert set(again._model.get_model_state()) == {"_W_data", "_W_indices", "_W_indptr", "_similarity", "_num_neighbors", "_implicit"}


def test_reference_pickle_loads_and_recommends(ctx, tmp_path):
    """A checkpoint in the reference's format ({'_preds', '_similarity', '_num_neighbors', '_implicit'}) is restored and
    recommended from through el_dense_topk."""
    from elliot_amd.recommender import ItemKNN
    data, cfg = make_data(tmp_path)
    R = data.sp_i_train_ratings
    W = knn_ref.build_w(R, "item", 15, "cosine")
    preds = knn_ref.scores(R, W, "item")
    model = ItemKNN(data=data, config=cfg, params=params(neighbors=15, similarity="cosine", meta={"restore": True}))
    with open(model._saving_filepath, "wb") as f:
        pickle.dump({"_preds": preds.astype(np.float32), "_similarity": "cosine", "_num_neighbors": 15, "_implicit": False}, f)
    model.train()
    _, recs = model.get_recommendations(10)
    users = np.arange(data.num_users)
    idx, val = knn_ref.topk(preds, users, 10, excl=(R.indptr, R.indices))
    for u in users:
        assert [(i, np.float32(v)) for i, v in recs[data.private_users[u]]] == \
            [(data.private_items[i], np.float32(v)) for i, v in zip(idx[u], val[u])], u
