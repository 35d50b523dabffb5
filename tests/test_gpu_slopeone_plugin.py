"""GPU end-to-end: the SlopeOne plugin through RecMixin -- for EVERY user of every golden case the reference's own value list
(tests/golden/slopeone_ref.npz) bit for bit, the item ids wherever the value is unique, its checkpoints in both directions, its
name and its refusals."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd.dataset.dataset import DataSet, default_config
from tests.helpers import slopeone_ref

pytestmark = pytest.mark.gpu

UOFF, IOFF = 1000, 5000                       # public ids differ from private ones
CASES = ["int", "half", "cold_item", "one_rating", "split"]
_pred = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def params(**kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    return SimpleNamespace(meta=meta, **kw)


def config(tmp_path):
    cfg = default_config(top_k=10, cutoffs=[10, 5], simple_metrics=["nDCG", "Recall"], out_dir=str(tmp_path))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    return cfg


def fixture_data(tmp_path, g, tag):
    """The case's dict-order rows as the train file of a DataSet (public ids = fixture ids + offsets, every fixture id known
    to it, so an item nobody rated keeps its row), one unrated test item per user."""
    indptr, indices, ratings, U, I = slopeone_ref.case(g, tag)
    users = np.repeat(np.arange(U), np.diff(indptr))
    rs = np.random.RandomState(1)
    te_i = [rs.choice(np.setdiff1d(np.arange(I), indices[indptr[u]:indptr[u + 1]])) for u in range(U)]
    cfg = config(tmp_path)
    tr = (users + UOFF, indices.astype(np.int64) + IOFF, ratings)
    te = (np.arange(U) + UOFF, np.asarray(te_i) + IOFF, np.ones(U))
    data = DataSet(cfg, tr, te, public_users=np.arange(U) + UOFF, public_items=np.arange(I) + IOFF)
    assert (data.num_users, data.num_items) == (U, I)
    return data, cfg


def unmasked_predictions(g, tag):
    """(pred [U, I], allowed [U, I]) of a case from the restatement: computed once, shared, never written to."""
    if tag not in _pred:
        indptr, indices, ratings, U, I = slopeone_ref.case(g, tag)
        freq, dev, mean = slopeone_ref.build(indptr, indices, ratings, U, I)
        allowed = np.ones((U, I), dtype=bool)
        allowed[np.repeat(np.arange(U), np.diff(indptr)), indices] = False
        _pred[tag] = slopeone_ref.predictions(indptr, indices, freq, dev, mean), allowed
    return _pred[tag]


def check_lists(recs, g, tag):
    """Every user's values equal the reference's bit for bit; ids are compared where the value is unique among the user's
    unmasked predictions (at ties the reference's argpartition order is arbitrary, ours is index-ascending)."""
    ref_idx, ref_val = g[f"{tag}_rec_idx"], g[f"{tag}_rec_val"]
    pred, allowed = unmasked_predictions(g, tag)
    compared = 0
    for u in range(ref_idx.shape[0]):
        lst = recs[u + UOFF]
        n = int((ref_idx[u] >= 0).sum())
        assert len(lst) == n, u
        assert np.array_equal(bits([v for _, v in lst]), bits(ref_val[u, :n])), u
        vals = pred[u][allowed[u]]
        for (item, v), ri in zip(lst, ref_idx[u, :n]):
            if (vals == v).sum() == 1:
                assert item - IOFF == int(ri), u
                compared += 1
    assert compared > 0.9 * ref_idx.size


@pytest.mark.parametrize("tag", CASES)
def test_lists_equal_reference(ctx, golden, tmp_path, tag):
    from elliot_amd.recommender import SlopeOne
    g = golden("slopeone_ref.npz")
    data, cfg = fixture_data(tmp_path, g, tag)
    model = SlopeOne(data=data, config=cfg, params=params())
    assert model.name == "SlopeOne"
    model.train()
    assert len(model._results) == 1
    _, recs = model.get_recommendations(10)
    check_lists(recs, g, tag)


@pytest.mark.parametrize("tag", ["half", "split"])
def test_save_restore_round_trip(ctx, golden, tmp_path, tag):
    from elliot_amd.recommender import SlopeOne
    g = golden("slopeone_ref.npz")
    data, cfg = fixture_data(tmp_path, g, tag)
    model = SlopeOne(data=data, config=cfg, params=params(meta={"save_weights": True}))
    model.train()
    with open(model._saving_filepath, "rb") as f:
        state = pickle.load(f)
    assert list(state) == ["freq", "dev", "user_mean"]
    assert state["freq"].dtype == np.float64 and np.array_equal(state["freq"], g[f"{tag}_freq"])
    assert state["dev"].dtype == np.float64 and np.array_equal(bits(state["dev"]), bits(g[f"{tag}_dev"]))
    assert isinstance(state["user_mean"], list) and all(type(x) is np.float64 for x in state["user_mean"])
    assert np.array_equal(bits(state["user_mean"]), bits(g[f"{tag}_user_mean"]))
    before = model.get_recommendations(10)[1]
    again = SlopeOne(data=data, config=cfg, params=params(meta={"restore": True}))
    assert again._model.state.T is None
    again.train()
    assert again.get_recommendations(10)[1] == before


@pytest.mark.parametrize("tag", ["int", "split"])
def test_reference_checkpoint_loads(ctx, golden, tmp_path, tag):
    """A pickle in the reference's own format (float64 freq and dev, a list of np.float64), written from the golden arrays."""
    from elliot_amd.recommender import SlopeOne
    g = golden("slopeone_ref.npz")
    data, cfg = fixture_data(tmp_path, g, tag)
    model = SlopeOne(data=data, config=cfg, params=params(meta={"restore": True}))
    os.makedirs(os.path.dirname(model._saving_filepath), exist_ok=True)
    with open(model._saving_filepath, "wb") as f:
        pickle.dump({"freq": g[f"{tag}_freq"], "dev": g[f"{tag}_dev"], "user_mean": [np.float64(x) for x in g[f"{tag}_user_mean"]]}, f)
    model.train()
    _, recs = model.get_recommendations(10)
    check_lists(recs, g, tag)


def test_dict_route_equals_device_route(ctx, golden, tmp_path):
    from elliot_amd.recommender import SlopeOne
    data, cfg = fixture_data(tmp_path, golden("slopeone_ref.npz"), "int")
    model = SlopeOne(data=data, config=cfg, params=params())
    assert model._device_metrics()
    model.train()
    device = model._results[-1][10]["test_results"]["nDCG"]
    host = model.evaluator.eval(model.get_recommendations(10))[10]["test_results"]["nDCG"]
    assert 0.0 <= device <= 1.0 and abs(device - host) < 1e-9


def test_oversize_catalogue_refused_before_allocation(ctx, tmp_path):
    from elliot_amd.recommender import SlopeOne
    I = 200_000                                               # 20 I^2 bytes = 800 GB
    cfg = config(tmp_path)
    tr = (np.repeat([1, 2], I // 2), np.arange(I) + IOFF, np.ones(I))
    te = (np.array([1, 2]), np.array([IOFF + 1, IOFF]), np.ones(2))
    data = DataSet(cfg, tr, te)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(ctx.device)
    with pytest.raises(ValueError, match="bytes"):
        SlopeOne(data=data, config=cfg, params=params())
    assert torch.cuda.memory_allocated(ctx.device) == before


def test_non_half_step_ratings_refused(ctx, golden, tmp_path):
    from elliot_amd.recommender import SlopeOne
    indptr, indices, ratings, U, I = slopeone_ref.case(golden("slopeone_ref.npz"), "int")
    cfg = config(tmp_path)
    users = np.repeat(np.arange(U), np.diff(indptr))
    data = DataSet(cfg, (users, indices.astype(np.int64), ratings + 0.3), (np.arange(U), np.zeros(U, np.int64), np.ones(U)))
    with pytest.raises(ValueError, match="SlopeOne needs integer or half-step"):
        SlopeOne(data=data, config=cfg, params=params())
