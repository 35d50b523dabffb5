"""GPU end-to-end: the PureSVD plugin through RecMixin -- the reference's lists (tests/golden/puresvd_ref.npz), the dict and
device-metric routes, sampled negatives, recs on disk, its checkpoint, its refusals and the sample config through the mini runner."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.synthetic import small_dataset
from tests.helpers import psvd_ref

pytestmark = pytest.mark.gpu

UOFF, IOFF = 1000, 5000                       # public ids differ from private ones
CASES = ["u300_i200_f10_s42", "u200_i320_f10_s42", "u400_i250_f32_s42", "u150_i120_f16_s42", "u1000_i600_f50_s42",
         "u600_i900_f100_s42", "u150_i120_f16_s7"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(**kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    return SimpleNamespace(meta=meta, **kw)


def config(tmp_path):
    cfg = default_config(top_k=10, cutoffs=[10, 5], simple_metrics=["nDCG", "Recall"], out_dir=str(tmp_path))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    return cfg


def fixture_data(tmp_path, A):
    """The fixture's train matrix as a DataSet (public ids = fixture ids + offsets), one unrated test item per user.  The private
    order is pinned to the fixture's: the start matrix is drawn per private column, so the reference's result -- recorded on the
    fixture as it stands -- belongs to that order (a loader that numbers the items otherwise gives the reference another draw)."""
    U, I = A.shape
    users = np.repeat(np.arange(U), np.diff(A.indptr))
    rs = np.random.RandomState(1)
    te_i = [rs.choice(np.setdiff1d(np.arange(I), A.indices[A.indptr[u]:A.indptr[u + 1]])) for u in range(U)]
    cfg = config(tmp_path)
    tr = (users + UOFF, A.indices + IOFF, np.ones(A.nnz))
    te = (np.arange(U) + UOFF, np.asarray(te_i) + IOFF, np.ones(U))
    data = DataSet(cfg, tr, te, public_users=np.arange(U) + UOFF, public_items=np.arange(I) + IOFF)
    assert (sp.csr_matrix(data.sp_i_train) != A).nnz == 0
    return data, cfg


def synthetic_data(tmp_path, n_users=260, n_items=200, seed=6):
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
    cfg = config(tmp_path)
    tr = (users[~flag] + UOFF, indices[~flag] + IOFF, ratings[~flag])
    te = (users[flag] + UOFF, indices[flag] + IOFF, ratings[flag])
    return DataSet(cfg, tr, te), cfg


@pytest.mark.parametrize("tag", CASES)
def test_lists_equal_reference(ctx, golden, tmp_path, tag):
    """get_recommendations(10) against the float32 reference's lists for every user whose list its float32 rounding does not
    decide (psvd_ref.fragile: a gap in the top 11 within four times the row's |P_ref32 - P_ref64|); at most 2 % may be."""
    from elliot_amd.recommender import PureSVD
    g = golden("puresvd_ref.npz")
    A = psvd_ref.csr_of(g, tag)
    data, cfg = fixture_data(tmp_path, A)
    assert (data.num_users, data.num_items) == A.shape
    assert all(data.public_users[u + UOFF] == u for u in (0, A.shape[0] - 1))
    model = PureSVD(data=data, config=cfg, params=params(factors=int(g[f"{tag}_factors"]), seed=int(g[f"{tag}_seed"])))
    model.train()
    _, recs = model.get_recommendations(10)
    P64 = psvd_ref.scores(*psvd_ref.ref64_tables(g, tag, A))
    weak = psvd_ref.fragile(P64, g[f"{tag}_row_err"], A.indptr, A.indices, 10)
    print(f"{tag}: fragile users {int(weak.sum())} of {A.shape[0]}")
    assert weak.sum() <= 0.02 * A.shape[0]
    ref = psvd_ref.ref32_lists(g, tag)
    bad = [u for u in np.flatnonzero(~weak) if [i - IOFF for i, _ in recs[u + UOFF]] != [int(i) for i in ref[u] if i >= 0]]
    assert not bad, (tag, bad[:10])


def test_dict_route_equals_device_route_and_predict(ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = synthetic_data(tmp_path)
    model = PureSVD(data=data, config=cfg, params=params(factors=20))
    assert model._device_metrics()
    model.train()
    assert len(model._results) == 1
    device = model._results[-1][10]["test_results"]["nDCG"]
    recs = model.get_recommendations(10)
    host = model.evaluator.eval(recs)[10]["test_results"]["nDCG"]
    assert 0.0 < device <= 1.0 and abs(device - host) < 1e-9
    user, lst = next(iter(recs[1].items()))
    for item, score in lst[:3]:                               # predict() takes public ids and is the listed score up to float32 summation order
        assert abs(model.predict(user, item) - score) <= 1e-5 * max(1.0, abs(score))


def test_train_writes_recs_when_asked(ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = synthetic_data(tmp_path)
    model = PureSVD(data=data, config=cfg, params=params(factors=12, meta={"save_recs": True}))
    assert not model._device_metrics()
    model.train()
    path = os.path.join(cfg.path_output_rec_result, "PureSVD_factors=12.tsv")
    assert os.path.getsize(path) > 0
    with open(path) as f:
        first = f.readline().split("\t")
    assert int(first[0]) >= UOFF and int(first[1]) >= IOFF


def test_save_restore_round_trip(ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = synthetic_data(tmp_path)
    model = PureSVD(data=data, config=cfg, params=params(factors=16, meta={"save_weights": True}))
    model.train()
    with open(model._saving_filepath, "rb") as f:
        state = pickle.load(f)
    assert set(state) == {"user_vec", "item_vec"}                       # the reference's keys
    assert state["user_vec"].dtype == np.float32 and state["user_vec"].shape == (data.num_users, 16)
    assert state["item_vec"].dtype == np.float32 and state["item_vec"].shape == (data.num_items, 16)
    before = model.get_recommendations(10)[1]
    again = PureSVD(data=data, config=cfg, params=params(factors=16, meta={"restore": True}))
    again.train()
    assert again.get_recommendations(10)[1] == before
    assert again._model.get_model_state()["user_vec"].tobytes() == state["user_vec"].tobytes()


def test_sampled_negatives(ctx, tmp_path):
    import yaml
    from elliot_amd import run as runner
    os.makedirs(tmp_path / "cfg")
    indptr, indices, _ = small_dataset(180, 260, seed=5)
    rs = np.random.RandomState(5)
    users = np.repeat(np.arange(180), np.diff(indptr))
    with open(tmp_path / "cfg" / "dataset.tsv", "w") as f:
        for u, i in zip(users, indices):
            f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "negative_sampling": {"strategy": "random", "num_items": 40},
           "top_k": 10, "evaluation": {"simple_metrics": ["nDCG", "HR"]},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/",
           "models": {"external.PureSVD": {"meta": {"save_recs": False}, "factors": 16}}}
    with open(tmp_path / "cfg" / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    res = runner.run_experiment(str(tmp_path / "cfg" / "exp.yml"))
    (name, r), = res.items()
    assert name == "PureSVD_factors=16"
    assert 0.0 < r[10]["test_results"]["HR"] <= 1.0
    cfg = runner.build_config(exp, str(tmp_path / "cfg"))
    data = runner.load_data(exp, cfg, str(tmp_path / "cfg"))
    from elliot_amd.recommender import PureSVD
    model = PureSVD(data=data, config=cfg, params=params(factors=16))
    model.train()
    dict_route = model.evaluator.eval(model.get_recommendations(10))
    assert abs(dict_route[10]["test_results"]["nDCG"] - model.get_results()[10]["test_results"]["nDCG"]) < 1e-9
    _, recs = model.get_recommendations(10)
    test_cand = model.get_candidate_mask()[1]
    ip, ix = test_cand.indptr.cpu().numpy(), test_cand.indices.cpu().numpy()
    pi = {v: k for k, v in data.private_items.items()}
    for u, lst in recs.items():
        pu = data.public_users[u]
        allowed = set(ix[ip[pu]:ip[pu + 1]].tolist())
        assert {pi[i] for i, _ in lst} <= allowed, u


def test_rank_deficient_input_is_refused(ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    rs = np.random.RandomState(8)
    base = rs.rand(12, 90) < 0.3                              # 200 users drawn from 12 distinct rows: rank <= 12 < 20
    base[np.arange(12), rs.randint(0, 90, 12)] = True
    base[rs.randint(0, 12, 90), np.arange(90)] = True
    dense = base[np.concatenate([np.arange(12), rs.randint(0, 12, 188)])]
    u, i = np.nonzero(dense)
    te_i = np.array([rs.choice(np.flatnonzero(~dense[x])) for x in range(200)])
    cfg = config(tmp_path)
    data = DataSet(cfg, (u + UOFF, i + IOFF, np.ones(u.shape[0])), (np.arange(200) + UOFF, te_i + IOFF, np.ones(200)))
    model = PureSVD(data=data, config=cfg, params=params(factors=10))
    with pytest.raises(ValueError, match=r"column \d+ of 20.*rank"):
        model.train()


def test_factors_too_large_are_refused(ctx, tmp_path):
    from elliot_amd.recommender import PureSVD
    data, cfg = synthetic_data(tmp_path)
    for factors, pattern in ((0, ">= 1"), (247, "at most 256"), (min(data.num_users, data.num_items) - 9, "exceeds min")):
        with pytest.raises(ValueError, match=pattern):
            PureSVD(data=data, config=cfg, params=params(factors=factors))


def test_sample_config_model_block_through_the_mini_runner(ctx, tmp_path):
    """config_files/sample_puresvd_amd.yml's model block, under both keys, on a synthetic data set."""
    import yaml
    from elliot_amd.run import run_experiment
    with open(os.path.join(REPO, "config_files", "sample_puresvd_amd.yml")) as f:
        block = yaml.safe_load(f)["experiment"]["models"]["PureSVD"]
    indptr, indices, _ = small_dataset(250, 200, seed=11)
    rs = np.random.RandomState(11)
    users = np.repeat(np.arange(250), np.diff(indptr))
    with open(tmp_path / "dataset.tsv", "w") as f:
        for u, i in zip(users, indices):
            f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")
    cfg = {"experiment": {
        "dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
        "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
        "top_k": 10, "evaluation": {"simple_metrics": ["nDCG"]},
        "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/",
        "path_output_rec_performance": "out/perf/",
        "models": {"PureSVD": dict(block), "external.PureSVD": {**block, "factors": 20}}}}
    with open(tmp_path / "exp.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    res = run_experiment(str(tmp_path / "exp.yml"))
    assert set(res) == {f"PureSVD_factors={block['factors']}", "PureSVD_factors=20"}
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["nDCG"] <= 1.0
    recs = sorted(os.listdir(tmp_path / "out" / "recs"))
    assert recs == sorted(f"{n}.tsv" for n in res)
