"""GPU end-to-end: the RP3beta plugin through the mini runner and the plugin surface (graph_based/RP3beta/rp3beta.py)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.synthetic import small_dataset
from tests.helpers import knn_ref, rp3_ref

pytestmark = pytest.mark.gpu

# get_params_shortcut writes a decimal point as '$', as the reference does
REF_NAME = "RP3beta_neighborhood=30_alpha=1$0_beta=0$6_normalize_similarity=False"
EXT_NAME = "RP3beta_neighborhood=20_alpha=0$8_beta=0$3_normalize_similarity=True"


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


def test_mini_runner_both_keys(ctx, tmp_path):
    import yaml
    from elliot_amd.run import run_experiment
    write_tsv(tmp_path / "dataset.tsv", 250, 200, seed=11)
    cfg = {"experiment": {
        "dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
        "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
        "top_k": 10, "evaluation": {"simple_metrics": ["nDCG"]},
        "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/",
        "path_output_rec_performance": "out/perf/",
        "models": {"RP3beta": {"meta": {"save_recs": True}, "neighborhood": 30},
                   "external.RP3beta": {"meta": {"save_recs": True}, "neighborhood": 20, "alpha": 0.8, "beta": 0.3,
                                        "normalize_similarity": True}}}}
    with open(tmp_path / "exp.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    res = run_experiment(str(tmp_path / "exp.yml"))
    assert set(res) == {REF_NAME, EXT_NAME}                      # names as the reference forms them
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["nDCG"] <= 1.0
    recs = sorted(os.listdir(tmp_path / "out" / "recs"))
    assert recs == sorted(f"{n}.tsv" for n in res)
    assert os.path.getsize(tmp_path / "out" / "recs" / f"{REF_NAME}.tsv") > 0


def test_dict_route_equals_device_route(ctx, tmp_path):
    from elliot_amd.recommender import RP3beta
    data, cfg = make_data(tmp_path)
    model = RP3beta(data=data, config=cfg, params=params(neighborhood=25))
    assert model._device_metrics()
    model.train()
    device = model.get_results()[10]["test_results"]["nDCG"]
    host = model.evaluator.eval(model.get_recommendations(10))[10]["test_results"]["nDCG"]
    assert 0.0 < device <= 1.0 and abs(device - host) < 1e-9


@pytest.mark.parametrize("alpha,beta,normalize", [(1.0, 0.6, False), (0.8, 0.3, True), (1.0, 0.0, False)])
def test_lists_equal_restatement(ctx, tmp_path, alpha, beta, normalize):
    """W and the lists of the plugin are the restatement's, computed in the same process (the same host np.power)."""
    from elliot_amd.recommender import RP3beta
    data, cfg = make_data(tmp_path)
    model = RP3beta(data=data, config=cfg, params=params(neighborhood=25, alpha=alpha, beta=beta, normalize_similarity=normalize))
    model.train()
    R = data.sp_i_train_ratings
    W = rp3_ref.build(R, 25, alpha, beta, normalize)
    Wd = model._model.w_csr()
    assert np.array_equal(Wd.indptr, W.indptr) and np.array_equal(Wd.indices, W.indices)
    assert np.array_equal(rp3_ref.bits(Wd.data), rp3_ref.bits(W.data))
    _, recs = model.get_recommendations(10)
    users = np.arange(data.num_users)
    idx, val = knn_ref.topk(knn_ref.scores(R, W, "item"), users, 10, excl=(R.indptr, R.indices))
    for u in users:
        exp = [(data.private_items[i], np.float32(v)) for i, v in zip(idx[u], val[u]) if i >= 0]
        got = recs[data.private_users[u]]
        assert [(i, np.float32(v)) for i, v in got] == exp, u


def test_neighborhood_minus_one_is_every_item(ctx, tmp_path):
    from elliot_amd.recommender import RP3beta
    data, cfg = make_data(tmp_path)
    model = RP3beta(data=data, config=cfg, params=params(neighborhood=-1, beta=0.0))
    assert model._neighborhood == data.num_items
    assert model.name == f"RP3beta_neighborhood={data.num_items}_alpha=1$0_beta=0$0_normalize_similarity=False"
    model.train()
    W = rp3_ref.build(data.sp_i_train_ratings, -1, 1.0, 0.0, False)
    assert model._model.w_csr().nnz == W.nnz


def test_save_restore_round_trip(ctx, tmp_path):
    from elliot_amd.recommender import RP3beta
    data, cfg = make_data(tmp_path)
    model = RP3beta(data=data, config=cfg, params=params(neighborhood=15, normalize_similarity=True, meta={"save_weights": True}))
    model.train()
    assert os.path.exists(model._saving_filepath)
    before = model.get_recommendations(10)[1]
    again = RP3beta(data=data, config=cfg, params=params(neighborhood=15, normalize_similarity=True, meta={"restore": True}))
    again.train()
    assert again.get_recommendations(10)[1] == before
    assert set(again._model.get_model_state()) == {"_W_data", "_W_indices", "_W_indptr", "_neighborhood", "_alpha", "_beta",
                                                   "_normalize_similarity"}
