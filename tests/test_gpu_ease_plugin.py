"""GPU end-to-end: the EASER plugin through RecMixin -- the reference's lists (tests/golden/ease_ref.npz), the dict and
device-metric routes, sampled negatives, its checkpoint, its name and its refusals."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.synthetic import small_dataset
from tests.helpers import ease_ref

pytestmark = pytest.mark.gpu

UOFF, IOFF = 1000, 5000                       # public ids differ from private ones


def params(**kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    return SimpleNamespace(meta=meta, **kw)


def config(tmp_path):
    cfg = default_config(top_k=10, cutoffs=[10, 5], simple_metrics=["nDCG", "Recall"], out_dir=str(tmp_path))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    return cfg


def fixture_data(tmp_path, g, tag):
    """The fixture's train matrix as a DataSet (public ids = fixture ids + offsets), one unrated test item per user."""
    R = sp.csr_matrix((g[f"{tag}_R_data"], g[f"{tag}_R_indices"], g[f"{tag}_R_indptr"]), shape=tuple(g[f"{tag}_shape"]))
    U, I = R.shape
    users = np.repeat(np.arange(U), np.diff(R.indptr))
    rs = np.random.RandomState(1)
    te_u, te_i = [], []
    for u in range(U):
        free = np.setdiff1d(np.arange(I), R.indices[R.indptr[u]:R.indptr[u + 1]])
        te_u.append(u)
        te_i.append(rs.choice(free))
    cfg = config(tmp_path)
    tr = (users + UOFF, R.indices + IOFF, R.data.astype(float))
    te = (np.asarray(te_u) + UOFF, np.asarray(te_i) + IOFF, np.ones(U))
    return DataSet(cfg, tr, te), cfg, R


def synthetic_data(tmp_path, n_users=260, n_items=200, seed=6, values=None):
    indptr, indices, _ = small_dataset(n_users, n_items, seed=seed)
    rs = np.random.RandomState(4)
    U = indptr.shape[0] - 1
    users = np.repeat(np.arange(U), np.diff(indptr))
    ratings = rs.randint(1, 6, indices.shape[0]).astype(float) if values is None else values(rs, indices.shape[0])
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


def fragile(S, S2, excl, k):
    """Users whose top k + 1 (masked) scores under S hold a gap no larger than four times the row's largest difference between
    S and S2 (the scores of the same R under the reference's float32 B and under the fp64-derived B): their order is decided
    by the reference's float32 rounding."""
    out = np.zeros(S.shape[0], bool)
    for u in range(S.shape[0]):
        s = S[u].astype(np.float64).copy()
        s[excl[1][excl[0][u]:excl[0][u + 1]]] = -np.inf
        top = np.sort(s[np.isfinite(s)])[::-1][:k + 1]
        err = 4.0 * np.abs(S[u].astype(np.float64) - S2[u]).max()
        out[u] = top.size > 1 and np.min(np.diff(top[::-1])) <= err
    return out


@pytest.mark.parametrize("tag", ["rat_l5", "rat_l1320", "bin_l50"])
def test_lists_equal_reference(ctx, golden, tmp_path, tag):
    from elliot_amd.recommender import EASER
    g = golden("ease_ref.npz")
    data, cfg, R = fixture_data(tmp_path, g, tag)
    assert (data.num_users, data.num_items) == R.shape
    model = EASER(data=data, config=cfg, params=params(l2_norm=float(g[f"{tag}_l2"])))
    model.train()
    _, recs = model.get_recommendations(10)
    ref_idx = g[f"{tag}_rec_idx"]
    l2 = float(g[f"{tag}_l2"])
    weak = fragile(R.dot(g[f"{tag}_B"]), ease_ref.scores(R, ease_ref.weights_f64(R, l2)), (R.indptr, R.indices), 10)
    assert weak.mean() < 0.5
    checked = 0
    for u in range(R.shape[0]):
        if weak[u]:
            continue
        assert [i - IOFF for i, _ in recs[u + UOFF]] == [int(i) for i in ref_idx[u] if i >= 0], u
        checked += 1
    assert checked > 0


def test_dict_route_equals_device_route(ctx, tmp_path):
    from elliot_amd.recommender import EASER
    data, cfg = synthetic_data(tmp_path)
    model = EASER(data=data, config=cfg, params=params(l2_norm=50.0))
    assert model._device_metrics()
    model.train()
    assert len(model._results) == 1
    device = model._results[-1][10]["test_results"]["nDCG"]
    host = model.evaluator.eval(model.get_recommendations(10))[10]["test_results"]["nDCG"]
    assert 0.0 < device <= 1.0 and abs(device - host) < 1e-9


def test_name_matches_reference(ctx, tmp_path):
    from elliot_amd.recommender import EASER
    data, cfg = synthetic_data(tmp_path)
    model = EASER(data=data, config=cfg, params=params(l2_norm=1320))
    assert model.name == f"EASER_neighborhood={data.num_items}_l2_norm=1320$0"
    model = EASER(data=data, config=cfg, params=params())
    assert model.name == f"EASER_neighborhood={data.num_items}_l2_norm=1000$0"


def test_save_restore_round_trip(ctx, tmp_path):
    from elliot_amd.recommender import EASER
    data, cfg = synthetic_data(tmp_path)
    model = EASER(data=data, config=cfg, params=params(l2_norm=30.0, meta={"save_weights": True}))
    model.train()
    with open(model._saving_filepath, "rb") as f:
        state = pickle.load(f)
    assert set(state) == {"B", "l2_norm", "neighborhood"}
    assert state["B"].dtype == np.float32 and state["B"].shape == (data.num_items, data.num_items)
    before = model.get_recommendations(10)[1]
    again = EASER(data=data, config=cfg, params=params(l2_norm=30.0, meta={"restore": True}))
    again.train()
    assert again.get_recommendations(10)[1] == before


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
           "models": {"external.EASER": {"meta": {"save_recs": False}, "l2_norm": 200}}}
    with open(tmp_path / "cfg" / "exp.yml", "w") as f:
        yaml.safe_dump({"experiment": exp}, f)
    res = runner.run_experiment(str(tmp_path / "cfg" / "exp.yml"))
    (name, r), = res.items()
    assert name.startswith("EASER_neighborhood=") and name.endswith("_l2_norm=200$0")
    assert 0.0 < r[10]["test_results"]["HR"] <= 1.0
    cfg = runner.build_config(exp, str(tmp_path / "cfg"))
    data = runner.load_data(exp, cfg, str(tmp_path / "cfg"))
    from elliot_amd.recommender import EASER
    model = EASER(data=data, config=cfg, params=params(l2_norm=200))
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


def test_oversize_catalogue_refused_before_allocation(ctx, tmp_path):
    from elliot_amd.recommender import EASER
    I = 200_000                                               # 20 I^2 bytes = 800 GB
    cfg = config(tmp_path)
    tr = (np.repeat([1, 2], I // 2), np.arange(I) + IOFF, np.ones(I))
    te = (np.array([1, 2]), np.array([IOFF + 1, IOFF]), np.ones(2))
    data = DataSet(cfg, tr, te)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(ctx.device)
    with pytest.raises(ValueError, match="bytes"):
        EASER(data=data, config=cfg, params=params())
    assert torch.cuda.memory_allocated(ctx.device) == before


def test_non_integer_ratings_refused(ctx, tmp_path):
    from elliot_amd.recommender import EASER
    data, cfg = synthetic_data(tmp_path, values=lambda rs, n: rs.randint(1, 6, n) + 0.3)
    with pytest.raises(ValueError, match="half-step"):
        EASER(data=data, config=cfg, params=params())
