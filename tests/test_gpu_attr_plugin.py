"""GPU end-to-end: the AttributeItemKNN / AttributeUserKNN / VSM plug-ins on the golden attribute fixture, through RecMixin and
through the mini runner on the sample configuration."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

from tests.helpers import attr_fixture as fxm
from tests.helpers import attr_ref, knn_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20


@pytest.fixture(scope="module")
def fx(golden, tmp_path_factory):
    return fxm.load(golden("attr_ref.npz"), tmp_path_factory.mktemp("attr"))


def vsm_scores(z, up, ip):
    return attr_ref.vsm_scores(fxm.csr(z, f"vsm_{up}_U"), fxm.csr(z, f"vsm_{ip}_I"))


def params(**kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    return SimpleNamespace(meta=meta, **kw)


def expected_lists(fx, preds):
    R = fx.data.sp_i_train
    users = np.arange(fx.data.num_users)
    idx, val = knn_ref.topk(preds, users, 10, excl=(R.indptr, R.indices))
    return {fx.data.private_users[u]: [(fx.data.private_items[i], np.float32(v)) for i, v in zip(idx[u], val[u]) if i >= 0] for u in users}


def as_lists(recs):
    return {u: [(i, np.float32(v)) for i, v in lst] for u, lst in recs.items()}


KNN_CASES = [("AttributeItemKNN", {"similarity": "cosine"}), ("AttributeItemKNN", {"similarity": "dot", "implicit": True}),
             ("AttributeUserKNN", {"similarity": "cosine", "profile": "binary"}),
             ("AttributeUserKNN", {"similarity": "dot", "profile": "tfidf"}),
             ("AttributeUserKNN", {"similarity": "cosine", "profile": "tfidf", "implicit": True})]


def knn_restatement(fx, name, kw):
    R = fx.data.sp_i_train if kw.get("implicit") else fx.data.sp_i_train_ratings
    if name == "AttributeItemKNN":
        W = knn_ref.build_w(fxm.csr(fx.z, "aik_A"), "user", N, kw["similarity"])             # "user": the rows of the item matrix
        return knn_ref.scores(R, W, "item")
    W = attr_ref.build_w(fxm.csr(fx.z, f"auk_{kw['profile']}_A"), N, kw["similarity"])
    return knn_ref.scores(R, W, "user")


@pytest.mark.parametrize("name,kw", KNN_CASES)
def test_knn_plugins_train_evaluate_and_list_the_restatement(ctx, fx, name, kw):
    from elliot_amd import recommender as rec
    model = getattr(rec, name)(data=fx.data, config=fx.cfg, params=params(neighbors=N, **kw))
    assert model._device_metrics()
    model.train()
    device = model.get_results()[10]["test_results"]["nDCG"]
    recs = model.get_recommendations(10)
    assert 0.0 < device <= 1.0 and abs(device - model.evaluator.eval(recs)[10]["test_results"]["nDCG"]) < 1e-9
    assert as_lists(recs[1]) == expected_lists(fx, knn_restatement(fx, name, kw))


@pytest.mark.parametrize("up,ip", [(u, i) for u in ("binary", "tfidf") for i in ("binary", "tfidf")])
def test_vsm_lists_equal_the_restatement(ctx, fx, up, ip):
    from elliot_amd.recommender import VSM
    model = VSM(data=fx.data, config=fx.cfg, params=params(user_profile=up, item_profile=ip))
    model.train()
    assert 0.0 < model.get_results()[10]["test_results"]["nDCG"] <= 1.0
    assert as_lists(model.get_recommendations(10)[1]) == expected_lists(fx, vsm_scores(fx.z, up, ip))


@pytest.mark.parametrize("name,kw,state", [
    ("AttributeItemKNN", {"neighbors": N}, {"_W_data", "_W_indices", "_W_indptr", "_similarity", "_num_neighbors", "_implicit"}),
    ("AttributeUserKNN", {"neighbors": N, "profile": "tfidf"},
     {"_W_data", "_W_indices", "_W_indptr", "_similarity", "_num_neighbors", "_implicit"}),
    ("VSM", {}, {"_similarity"} | {f"{t}_{f}" for t in ("_A", "_B") for f in ("data", "indices", "indptr", "shape")})])
def test_save_restore_round_trip(ctx, fx, name, kw, state):
    from elliot_amd import recommender as rec
    cls = getattr(rec, name)
    model = cls(data=fx.data, config=fx.cfg, params=params(meta={"save_weights": True}, **kw))
    model.train()
    assert os.path.exists(model._saving_filepath)
    before = model.get_recommendations(10)[1]
    again = cls(data=fx.data, config=fx.cfg, params=params(meta={"restore": True}, **kw))
    for attr in ("_attribute_matrix", "_user_profile_matrix", "_item_attribute_matrix"):          # a restored model builds no matrix
        setattr(again._model, attr, None)
    again.train()
    assert again.get_recommendations(10)[1] == before
    assert set(again._model.get_model_state()) == state


@pytest.mark.parametrize("name,kw", [("AttributeItemKNN", {"similarity": "cosine"}),
                                     ("AttributeUserKNN", {"similarity": "cosine", "profile": "tfidf"})])
def test_reference_knn_pickle_restores(ctx, fx, name, kw):
    """A checkpoint in the reference's format holds the dense `_preds` (R.dot(W) / W.dot(R)); it is recommended from as it is."""
    from elliot_amd import recommender as rec
    preds = knn_restatement(fx, name, kw)
    model = getattr(rec, name)(data=fx.data, config=fx.cfg, params=params(neighbors=N, meta={"restore": True}, **kw))
    model._model._attribute_matrix = None                                                         # nothing is built
    with open(model._saving_filepath, "wb") as f:
        pickle.dump({"_preds": preds.astype(np.float32), "_similarity": "cosine", "_num_neighbors": N, "_implicit": False}, f)
    model.train()
    assert as_lists(model.get_recommendations(10)[1]) == expected_lists(fx, preds)


def test_reference_vsm_pickle_restores(ctx, fx):
    """VSM's checkpoint in the reference's format holds the similarity's name only, so the model is built again."""
    from elliot_amd.recommender import VSM
    vsm = VSM(data=fx.data, config=fx.cfg, params=params(meta={"restore": True}))
    with open(vsm._saving_filepath, "wb") as f:
        pickle.dump({"_similarity": "cosine"}, f)
    vsm.train()
    assert as_lists(vsm.get_recommendations(10)[1]) == expected_lists(fx, vsm_scores(fx.z, "tfidf", "tfidf"))


def test_mini_runner_on_the_sample_configuration(ctx, tmp_path):
    """The shipped yml beside the shipped sample data, copied as they are: its relative dataset and attribute paths go through the
    runner's own resolution.  Only the output folders are added (the yml leaves them at the runner's defaults)."""
    import shutil

    import yaml
    from elliot_amd.run import run_experiment
    shutil.copytree(os.path.join(ROOT, "config_files", "attribute_sample"), tmp_path / "config_files" / "attribute_sample")
    with open(os.path.join(ROOT, "config_files", "sample_attribute_knn_amd.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert not any(k.startswith("path_output") for k in cfg["experiment"])
    cfg["experiment"].update(path_output_rec_result="../out/recs/", path_output_rec_weight="../out/weights/",
                             path_output_rec_performance="../out/perf/")
    with open(tmp_path / "config_files" / "sample_attribute_knn_amd.yml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    res = run_experiment(str(tmp_path / "config_files" / "sample_attribute_knn_amd.yml"))
    assert set(res) == {"AttributeItemKNN_nn=40_sim=cosine_bin=False_load=ItemAttributes",
                        "AttributeUserKNN_nn=40_sim=cosine_profile=tfidf_bin=False_load=ItemAttributes",
                        "VSM_sim=cosine_up=tfidf_ip=tfidf_load=ItemAttributes"}
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["nDCG"] <= 1.0
    assert sorted(os.listdir(tmp_path / "out" / "recs")) == sorted(f"{n}.tsv" for n in res)
