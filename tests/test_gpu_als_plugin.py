"""GPU end-to-end: the iALS / WRMF plugins through RecMixin (dict and device-metric routes, sampled negatives), checkpoints
(their own and the reference's pickle format) and the refusals."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.synthetic import small_dataset
from tests.helpers import als_ref

pytestmark = pytest.mark.gpu


def make_data(tmp_path, n_users=260, n_items=200, seed=6):
    indptr, indices, _ = small_dataset(n_users, n_items, seed=seed)
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


MODELS = {"iALS": dict(epochs=3, factors=12, alpha=2.0, reg=0.1), "WRMF": dict(epochs=3, factors=12, alpha=1, reg=0.1)}


@pytest.mark.parametrize("model_name", list(MODELS))
def test_dict_route_equals_device_route(ctx, tmp_path, model_name):
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    model = getattr(rec, model_name)(data=data, config=cfg, params=params(**MODELS[model_name]))
    assert model._device_metrics()
    model.train()
    assert len(model._results) == 3
    device = model._results[-1][10]["test_results"]["nDCG"]          # the final tables (the best iteration may be an earlier one)
    host = model.evaluator.eval(model.get_recommendations(10))[10]["test_results"]["nDCG"]
    assert 0.0 < device <= 1.0 and abs(device - host) < 1e-9


@pytest.mark.parametrize("model_name", list(MODELS))
def test_lists_equal_restatement(ctx, tmp_path, model_name):
    """After training, the plugin's lists are the masked top-10 of X Y^T of its own tables (fragile users aside)."""
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    model = getattr(rec, model_name)(data=data, config=cfg, params=params(**MODELS[model_name]))
    model.train()
    _, recs = model.get_recommendations(10)
    X, Y = model._model.state.X.cpu().numpy(), model._model.state.Y.cpu().numpy()
    B = data.sp_i_train
    idx, _, S = als_ref.topk(X, Y, (B.indptr, B.indices), 10)
    fragile = als_ref.fragile_users(S, (B.indptr, B.indices), 10)
    for u in range(data.num_users):
        if not fragile[u]:
            assert [i for i, _ in recs[data.private_users[u]]] == [data.private_items[i] for i in idx[u]], u


def test_sampled_negatives_and_names(ctx, tmp_path):
    import yaml
    from elliot_amd import run as runner
    os.makedirs(tmp_path / "cfg")
    write_tsv(tmp_path / "cfg" / "dataset.tsv", 180, 260, seed=5)
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "negative_sampling": {"strategy": "random", "num_items": 40},
           "top_k": 10, "evaluation": {"simple_metrics": ["nDCG", "HR"]},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/",
           "models": {"iALS": {"meta": {"save_recs": False}, "epochs": 2, "factors": 16},
                      "external.WRMF": {"meta": {"save_recs": False}, "epochs": 2, "factors": 16, "alpha": 2}}}
    with open(tmp_path / "cfg" / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    res = runner.run_experiment(str(tmp_path / "cfg" / "exp.yml"))
    assert set(res) == {"iALS_seed=42_e=2_bs=-1_factors=16_alpha=1$0_epsilon=1$0_reg=0$1_scaling=linear",
                        "WRMF_seed=42_e=2_bs=-1_factors=16_alpha=2_reg=0$1"}
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["HR"] <= 1.0
    cfg = runner.build_config(exp, str(tmp_path / "cfg"))
    data = runner.load_data(exp, cfg, str(tmp_path / "cfg"))
    from elliot_amd.recommender import iALS
    model = iALS(data=data, config=cfg, params=params(epochs=2, factors=16))
    model.train()
    _, recs = model.get_recommendations(10)
    for u, lst in recs.items():
        assert not ({i for i, _ in lst} & set(data.train_dict[u])), u
    dict_route = model.evaluator.eval(model.get_recommendations(10))
    assert abs(dict_route[10]["test_results"]["nDCG"] - model.get_results()[10]["test_results"]["nDCG"]) < 1e-9


@pytest.mark.parametrize("model_name", list(MODELS))
def test_save_restore_round_trip(ctx, tmp_path, model_name):
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    cls = getattr(rec, model_name)
    kw = dict(MODELS[model_name], epochs=1)                              # one iteration: the saved (best) tables are the final ones
    model = cls(data=data, config=cfg, params=params(**kw, meta={"save_weights": True}))
    model.train()
    assert os.path.exists(model._saving_filepath)
    with open(model._saving_filepath, "rb") as f:
        state = pickle.load(f)
    assert set(state) == {"pred_mat", "X", "Y", "C"}
    assert sp.issparse(state["X"]) == (model_name == "WRMF") and sp.issparse(state["C"])
    before = model.get_recommendations(10)[1]
    again = cls(data=data, config=cfg, params=params(**kw, meta={"restore": True}))
    again.train()
    assert again.get_recommendations(10)[1] == before


@pytest.mark.parametrize("model_name", list(MODELS))
def test_reference_pickle_loads(ctx, tmp_path, model_name):
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    F = MODELS[model_name]["factors"]
    rs = np.random.RandomState(9)
    X, Y = rs.normal(size=(data.num_users, F)), rs.normal(size=(data.num_items, F))
    B = data.sp_i_train
    state = {"pred_mat": X.dot(Y.T), "X": X, "Y": Y, "C": B.copy()}
    if model_name == "WRMF":
        state.update(X=sp.csr_matrix(X), Y=sp.csr_matrix(Y))
    model = getattr(rec, model_name)(data=data, config=cfg, params=params(**MODELS[model_name], meta={"restore": True}))
    with open(model._saving_filepath, "wb") as f:
        pickle.dump(state, f)
    model.train()
    _, recs = model.get_recommendations(10)
    idx, _, S = als_ref.topk(X, Y, (B.indptr, B.indices), 10)
    fragile = als_ref.fragile_users(S, (B.indptr, B.indices), 10)
    for u in range(data.num_users):
        if not fragile[u]:
            assert [i for i, _ in recs[data.private_users[u]]] == [data.private_items[i] for i in idx[u]], u


@pytest.mark.parametrize("model_name,kw", [("iALS", dict(factors=129)), ("WRMF", dict(factors=129)), ("iALS", dict(alpha=-1.0)),
                                            ("WRMF", dict(alpha=-1)), ("iALS", dict(scaling="log", epsilon=0))])
def test_refusals(ctx, tmp_path, model_name, kw):
    from elliot_amd import recommender as rec
    data, cfg = make_data(tmp_path)
    with pytest.raises(ValueError):
        getattr(rec, model_name)(data=data, config=cfg, params=params(epochs=1, **kw))


def test_rank_deficient_without_reg_raises(ctx, tmp_path):
    """reg = 0 and three items for eight factors: every A_u = G + w_A S_u has rank <= 3."""
    from elliot_amd.recommender import WRMF
    data, cfg = make_data(tmp_path, n_users=80, n_items=3, seed=2)
    assert data.num_items <= 3
    model = WRMF(data=data, config=cfg, params=params(epochs=1, factors=8, reg=0))
    with pytest.raises(np.linalg.LinAlgError, match="row"):
        model.train()
