"""GPU end-to-end: the FISM plugin (recommender/latent_factor_models/FISM) on the ratings of config_files/attribute_sample/ for two
epochs through RecMixin.train() / evaluate(): the losses are finite, the lists of get_recommendations(10) are the top-10 items of
batch_predict restated in float64 from the model's own downloaded tables (wherever the float64 gap between ranks 10 and 11 exceeds
twice the bound of tests/test_gpu_fism.py, taken between a float64 and a float32 restatement), a checkpoint round trip gives the same
lists, and a non-integer neg_ratio is refused."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd import run as runner
from tests.helpers import fism_ref

pytestmark = pytest.mark.gpu

K = 10
SAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config_files", "attribute_sample")


def experiment(folder):
    os.makedirs(folder / "cfg", exist_ok=True)
    shutil.copy(os.path.join(SAMPLE, "dataset.tsv"), folder / "cfg" / "dataset.tsv")
    exp = {"dataset": "attribute_sample", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": K, "evaluation": {"simple_metrics": ["nDCG", "Recall"], "cutoffs": [K, 5]},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/"}
    cfg = runner.build_config(exp, str(folder / "cfg"))
    return runner.load_data(exp, cfg, str(folder / "cfg")), cfg


def params(**kw):
    base = dict(seed=42, epochs=2, batch_size=64, factors=10, lr=0.01, alpha=0.5, beta=0.001, gamma=0.001, neg_ratio=4)
    return SimpleNamespace(meta=SimpleNamespace(verbose=False), **{**base, "lambda": 0.001, **kw})


def dense_lists(model, data, pad):
    """Per user the float64 top-K of batch_predict among the candidates, from the model's own tables; and which users it decides."""
    st, w = model._model.state, model._model.get_model_state()
    hist = np.split(st.index[1].astype(np.int64), st.index[0][1:-1])
    case = SimpleNamespace(U=st.U, I=st.I, L=st.longest, hist=hist, coef=st.coef.cpu().numpy(), **{n: w[n] for n in fism_ref.NAMES})
    p64, p32 = (fism_ref.Model(case, dt, pad=pad).batch_predict().numpy().astype(np.float64) for dt in (torch.float64, torch.float32))
    tol = fism_ref.bound(p64, p32)
    s = np.where(data.sp_i_train.toarray() != 0, -np.inf, p64)
    order = np.argsort(-s, axis=1, kind="stable")
    top = np.take_along_axis(s, order, axis=1)
    return np.sort(order[:, :K], 1), (top[:, K - 1] - top[:, K]) > 2 * tol       # (the 10th/11th gap decides the ten items, not their order)


@pytest.mark.parametrize("padding,loss", [("reference", "reference"), ("none", "bce")])
def test_two_epochs_lists_and_a_checkpoint_round_trip(ctx, tmp_path, padding, loss):
    from elliot_amd import external, recommender
    assert external.FISM is recommender.FISM and "FISM" in recommender.__all__
    data, cfg = experiment(tmp_path)
    model = recommender.FISM(data=data, config=cfg, params=params(padding=padding, loss=loss))
    assert model.name.startswith("FISM_") and model._neg_ratio == 4 and model._model.state.pad_len == (model._model.state.longest if padding == "reference" else 0)
    model.train()
    assert len(model._losses) == 2 and np.isfinite(model._losses).all() and model._model.state.step > 2
    want, decided = dense_lists(model, data, padding == "reference")
    recs = model.get_recommendations(K)[1]
    got = np.array([[data.public_items[i] for i, _ in recs[data.private_users[u]]] for u in range(data.num_users)])
    assert decided.sum() > data.num_users // 2 and np.array_equal(np.sort(got[decided], 1), want[decided])
    path = str(tmp_path / "fism.pkl")
    model._model.save_weights(path)
    other = recommender.FISM(data=data, config=cfg, params=params(seed=7, padding=padding, loss=loss))
    assert not torch.equal(other._model.state.Gi, model._model.state.Gi)
    other._model.load_weights(path)
    mask = model.get_candidate_mask()
    a, b = model._model.recommend(mask, K, 0, data.num_users), other._model.recommend(mask, K, 0, data.num_users)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and other._model.state.step == model._model.state.step


@pytest.mark.parametrize("bad", [0.5, "2.5", 0])
def test_a_non_integer_neg_ratio_is_refused(ctx, tmp_path, bad):
    from elliot_amd.recommender import FISM
    data, cfg = experiment(tmp_path)
    with pytest.raises(Exception, match="neg_ratio"):
        FISM(data=data, config=cfg, params=params(neg_ratio=bad))
