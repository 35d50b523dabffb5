"""GPU end-to-end: the Slim plugin through the mini runner and the plugin surface (latent_factor_models/Slim/slim.py)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.synthetic import small_dataset
from tests.helpers import knn_ref, slim_ref

pytestmark = pytest.mark.gpu

# get_base_params_shortcut / get_params_shortcut write a decimal point as '$', as the reference does
REF_NAME = "Slim_seed=42_e=2_bs=-1_l1=0$1_alpha=0$01_neighborhood=30_excl=column"
EXT_NAME = "Slim_seed=42_e=2_bs=-1_l1=0$5_alpha=0$05_neighborhood=20_excl=reference"


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
        "models": {"Slim": {"meta": {"save_recs": True}, "neighborhood": 30, "alpha": 0.01, "l1_ratio": 0.1},
                   "external.Slim": {"meta": {"save_recs": True}, "neighborhood": 20, "alpha": 0.05, "l1_ratio": 0.5,
                                     "exclusion": "reference"}}}}
    with open(tmp_path / "exp.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    res = run_experiment(str(tmp_path / "exp.yml"))
    assert set(res) == {REF_NAME, EXT_NAME}                      # names as the reference forms them, plus the exclusion
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["nDCG"] <= 1.0
    recs = sorted(os.listdir(tmp_path / "out" / "recs"))
    assert recs == sorted(f"{n}.tsv" for n in res)
    assert os.path.getsize(tmp_path / "out" / "recs" / f"{REF_NAME}.tsv") > 0


def test_dict_route_equals_device_route(ctx, tmp_path):
    from elliot_amd.recommender import Slim
    data, cfg = make_data(tmp_path)
    model = Slim(data=data, config=cfg, params=params(neighborhood=25, alpha=0.01, l1_ratio=0.1))
    assert model._device_metrics()
    model.train()
    device = model.get_results()[10]["test_results"]["nDCG"]
    host = model.evaluator.eval(model.get_recommendations(10))[10]["test_results"]["nDCG"]
    assert 0.0 < device <= 1.0 and abs(device - host) < 1e-9


@pytest.mark.parametrize("exclusion", ["column", "reference"])
def test_lists_equal_the_scores_of_the_models_own_w(ctx, tmp_path, exclusion):
    """Scoring is exact given W, so the GPU's own W is the operand: the plugin's lists == topk(R W) on the host, exactly; and W
    itself is the restatement's within the tolerance rule (D_ref from the float32 and float64 restatements)."""
    from elliot_amd.recommender import Slim
    data, cfg = make_data(tmp_path)
    model = Slim(data=data, config=cfg, params=params(neighborhood=25, alpha=0.01, l1_ratio=0.1, exclusion=exclusion))
    model.train()
    R = sp.csr_matrix(data.sp_i_train_ratings, dtype=np.float32)
    W = model._model.w_csr()
    assert all((np.diff(W.indices[W.indptr[i]:W.indptr[i + 1]]) > 0).all() for i in range(W.shape[0]))     # columns ascending
    c32, _ = slim_ref.fit(R, 0.01, 0.1, 42, exclusion, np.float32)
    c64, _ = slim_ref.fit(R, 0.01, 0.1, 42, exclusion, np.float64)
    bound, d_ref = slim_ref.tolerance(c32, c64)
    Wr, _ = slim_ref.w_from_coef(c32, 25)
    fragile = slim_ref.compare_w(W, Wr, c32, bound)
    print(f"{exclusion}: D_ref {d_ref:.3g}, bound {bound:.3g}, fragile columns {fragile}/{W.shape[0]}")
    assert fragile <= W.shape[0] // 20
    _, recs = model.get_recommendations(10)
    users = np.arange(data.num_users)
    idx, val = knn_ref.topk(knn_ref.scores(R, W, "item"), users, 10, excl=(R.indptr, R.indices))
    for u in users:
        exp = [(data.private_items[i], np.float32(v)) for i, v in zip(idx[u], val[u]) if i >= 0]
        got = recs[data.private_users[u]]
        assert [(i, np.float32(v)) for i, v in got] == exp, u


def test_save_restore_round_trip(ctx, tmp_path):
    from elliot_amd.recommender import Slim
    data, cfg = make_data(tmp_path)
    kw = dict(neighborhood=15, alpha=0.01, l1_ratio=0.1)
    model = Slim(data=data, config=cfg, params=params(meta={"save_weights": True}, **kw))
    model.train()
    assert os.path.exists(model._saving_filepath)
    before = model.get_recommendations(10)[1]
    again = Slim(data=data, config=cfg, params=params(meta={"restore": True}, **kw))
    again.train()
    assert again.get_recommendations(10)[1] == before
    assert again._model.get_model_state()["_exclusion"] == "column"
    assert set(again._model.get_model_state()) == {"_W_data", "_W_indices", "_W_indptr", "_l1_ratio", "_alpha", "_neighborhood", "_seed",
                                                   "_exclusion"}


@pytest.mark.parametrize("tag", ["ref_a0.001_l0.001_n10", "ref_a0.01_l0.1_n10"])
def test_reference_exclusion_reproduces_the_reference_w(ctx, golden, tag):
    """`exclusion: reference` through the model class: the W of the reference's own SlimModel.train() within the tolerance rule
    (D_ref from sklearn's float32 and float64 weights in the golden); the kept index sets are equal except on fragile columns
    (the gap at the cut below the bound), at most 5 % of them."""
    from elliot_amd.recommender.latent_factor_models.Slim.slim_model import SlimModel
    z, R = slim_ref.load_golden(golden)
    _, alpha, l1_ratio, N, exclusion = [c for c in slim_ref.golden_cases(golden) if c[0] == tag][0]
    assert exclusion == "reference"
    I = R.shape[1]
    model = SlimModel(SimpleNamespace(sp_i_train_ratings=R), l1_ratio, alpha, N, int(z["seed"]), exclusion, ctx)
    model.initialize()
    W, Wg = model.w_csr(), slim_ref.golden_w(z, tag, I)
    c32 = slim_ref.golden_dense(z, f"{tag}_c32", I, np.float32)
    bound, _ = slim_ref.tolerance(c32, slim_ref.golden_dense(z, f"{tag}_c64", I, np.float64))
    fragile = slim_ref.compare_w(W, Wg, c32, bound)
    print(f"{tag}: fragile columns {fragile}/{I}")
    assert fragile <= I // 20


def test_unknown_exclusion_is_refused(ctx, tmp_path):
    from elliot_amd.recommender import Slim
    data, cfg = make_data(tmp_path)
    with pytest.raises(ValueError, match="exclusion"):
        Slim(data=data, config=cfg, params=params(exclusion="row"))
