"""GPU end-to-end: AUC, GAUC and LAUC through RecMixin (`evaluation.rank_metrics: True`) for one model of each scoring route --
fp32 tables (BPRMF_batch), fp64 tables (BPRMF), blocked dense scores (EASER) -- under the exclusion and the candidate protocol.

The reported values are compared with ranks.finish on positions READ OFF the model's own recommend(k = num_items) lists: the
per-user rows are the same integers and IEEE divisions on either side, the sums are taken in two orders (bound 1e-11
max(1, |ref|), rank_ref.TOL).  nDCG must be the very number the evaluator gives without the rank metrics."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest

from elliot_amd import run as runner
from elliot_amd.evaluation import ranks
from elliot_amd.evaluation.evaluator import Evaluator
from tests.helpers import rank_ref

pytestmark = pytest.mark.gpu

U, I = 200, 300
METRICS = ["nDCG", "AUC", "GAUC", "LAUC"]
MODELS = {"BPRMF_batch": dict(epochs=1, batch_size=512, factors=16, lr=0.01),
          "BPRMF": dict(epochs=1, factors=8),
          "EASER": dict(l2_norm=10.0)}


def experiment(folder, negative_sampling, metrics=METRICS, gate=True):
    rs = np.random.RandomState(11)
    os.makedirs(folder / "cfg", exist_ok=True)
    with open(folder / "cfg" / "dataset.tsv", "w") as f:
        for u in range(U):
            for i in rs.choice(I, rs.randint(8, 40), replace=False):
                f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")
    ev = {"simple_metrics": list(metrics), "cutoffs": [10, 5], "relevance_threshold": 3}
    if gate:
        ev["rank_metrics"] = True
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": 10, "evaluation": ev,
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/"}
    if negative_sampling:
        exp["negative_sampling"] = {"strategy": "random", "num_items": 40}
    cfg = runner.build_config(exp, str(folder / "cfg"))
    return runner.load_data(exp, cfg, str(folder / "cfg")), cfg


def params(name, **meta):
    return SimpleNamespace(meta=SimpleNamespace(verbose=False, **meta), seed=42, **MODELS[name])


def positions_from_lists(model, data):
    """The position of every held-out entry in the model's own full-length list (entries at -inf and pads are not part of it)."""
    n_items = data.num_items
    idx, val = model._model.recommend(model.get_candidate_mask(), n_items, 0, data.num_users)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    tp, tc, _ = data.split_csr(False)
    pos = np.full(tc.shape[0], -1, dtype=np.int32)
    for u in range(data.num_users):
        live = (idx[u] >= 0) & np.isfinite(val[u])
        assert live[:int(live.sum())].all()                                     # the live entries are a prefix
        place = {int(i): q for q, i in enumerate(idx[u][live])}
        for e in range(tp[u], tp[u + 1]):
            pos[e] = place.get(int(tc[e]), -1)
    return pos


@pytest.mark.parametrize("negative_sampling", [False, True], ids=["excl", "cand"])
@pytest.mark.parametrize("name", list(MODELS))
def test_reported_rank_metrics_equal_the_models_own_full_lists(ctx, tmp_path, name, negative_sampling):
    from elliot_amd import recommender as rec
    data, cfg = experiment(tmp_path, negative_sampling)
    assert abs(data.num_users - U) <= 2 and data.num_items <= I
    model = getattr(rec, name)(data=data, config=cfg, params=params(name))
    assert model.evaluator.get_needed_recommendations() == 10
    ctx.timing(True)
    try:
        model.train()
        kernels = set(ctx.timing_report())
    finally:
        ctx.timing(False)
    assert "k_rank_metrics" in kernels and kernels & {"k_rank_wave", "k_rank_wave_f64", "k_score_rank_mfma"}
    res = model.get_results()
    pos = positions_from_lists(model, data)
    tp, tc, tr = data.split_csr(False)
    assert (pos[tc < data.num_items] >= 0).all()                                # a held-out item with a model row is always ranked
    train_len = np.diff(data.sp_i_train.tocsr().indptr)
    # without the rank metrics: the same lists through an evaluator that knows nothing of them
    plain = copy.copy(data)
    plain.config = copy.deepcopy(cfg)
    plain.config.evaluation.simple_metrics = ["nDCG"]
    del plain.config.evaluation.rank_metrics
    idx, _ = model._model.recommend(model.get_candidate_mask(), 10, 0, data.num_users)
    plain_res = Evaluator(plain, None).eval_device(ctx, plain, [(0, idx, idx)])
    for c in (10, 5):
        got = res[c]["test_results"]
        assert list(got) == METRICS
        want, sums = ranks.finish(pos, tp, tr, 3, train_len, data.num_items, c)
        assert sums[4] > 0.5 * data.num_users and sums[5] == 0
        rank_ref.check_values(got, [want[m] for m in rank_ref.NAMES], f"{name}@{c}")
        assert got["nDCG"] == plain_res[c]["test_results"]["nDCG"]
        assert 0.0 < got["AUC"] < 1.0 and 0.0 < got["GAUC"] < 1.0


def test_save_recs_still_writes_the_lists_and_the_metrics_come_from_the_device(ctx, tmp_path):
    from elliot_amd.recommender import BPRMF_batch
    data, cfg = experiment(tmp_path, False)
    model = BPRMF_batch(data=data, config=cfg, params=params("BPRMF_batch", save_recs=True))
    model.train()
    written = os.listdir(cfg.path_output_rec_result)
    assert len(written) == 1 and os.path.getsize(os.path.join(cfg.path_output_rec_result, written[0])) > 0
    assert list(model.get_results()[10]["test_results"]) == METRICS


def test_models_outside_the_wired_set_and_the_host_route_raise_at_construction(ctx, tmp_path):
    from elliot_amd.recommender import BPRMF_batch, ItemKNN
    data, cfg = experiment(tmp_path, False)
    with pytest.raises(Exception, match="ItemKNN cannot evaluate AUC, GAUC, LAUC"):
        ItemKNN(data=data, config=cfg, params=SimpleNamespace(meta=SimpleNamespace(verbose=False), neighbors=10, similarity="cosine"))
    cfg.device_metrics = False
    with pytest.raises(Exception, match="device_metrics: False"):
        BPRMF_batch(data=data, config=cfg, params=params("BPRMF_batch"))
