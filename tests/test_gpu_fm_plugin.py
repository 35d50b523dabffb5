"""GPU end-to-end: the FM plugin (recommender/latent_factor_models/FM) on config_files/attribute_sample/ for two epochs through
RecMixin.train(): the loss falls, the lists of get_recommendations(10) are the top-10 of a float64 dense recomputation of y^ from
the model's own downloaded tables (wherever the float64 gap between ranks 10 and 11 exceeds twice the bound of tests/test_gpu_fm.py,
taken between a float64 and a float32 recomputation), and a checkpoint round trip gives the same lists."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd import run as runner
from tests.helpers import fm_ref

pytestmark = pytest.mark.gpu

K = 10
SAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config_files", "attribute_sample")


def experiment(folder, attributes=True):
    os.makedirs(folder / "cfg", exist_ok=True)
    for name in ("dataset.tsv", "item_attributes.tsv"):
        shutil.copy(os.path.join(SAMPLE, name), folder / "cfg" / name)
    side = [{"dataloader": "ItemAttributes", "attribute_file": "item_attributes.tsv"}] if attributes else []
    exp = {"dataset": "attribute_sample", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv", "side_information": side},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": K, "evaluation": {"simple_metrics": ["nDCG", "Recall"], "cutoffs": [K, 5]},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/"}
    cfg = runner.build_config(exp, str(folder / "cfg"))
    return runner.load_data(exp, cfg, str(folder / "cfg")), cfg


def params(**kw):
    return SimpleNamespace(meta=SimpleNamespace(verbose=False), **{**dict(seed=42, epochs=2, batch_size=64, factors=10, lr=0.01, reg=0.1), **kw})


def dense_lists(model, data):
    """Per user the float64 top-K among the candidates, from the model's own tables; and which users the scores decide."""
    st = model._model.state
    w = model._model.get_model_state()
    case = SimpleNamespace(U=st.U, I=st.I, nF=st.nF, F=st.F, E=w["E"], w=w["w"], g0=w["g0"][0],
                           feats=model._item_features or [[] for _ in range(st.I)])
    p64, p32 = (fm_ref.Model(case, dt).predict_all().numpy().astype(np.float64) for dt in (torch.float64, torch.float32))
    tol = fm_ref.bound(p64, p32)
    s = np.where(data.sp_i_train.toarray() != 0, -np.inf, p64)
    order = np.argsort(-s, axis=1, kind="stable")
    top = np.take_along_axis(s, order, axis=1)
    return order[:, :K], (top[:, K - 1] - top[:, K]) > 2 * tol


@pytest.mark.parametrize("attributes", [True, False])
def test_two_epochs_lists_and_a_checkpoint_round_trip(ctx, tmp_path, attributes):
    from elliot_amd.recommender import FM
    data, cfg = experiment(tmp_path, attributes)
    model = FM(data=data, config=cfg, params=params())
    assert model.name.startswith("FM_") and (model._nfeatures > 0) == attributes
    if attributes:
        side = data.side_information.ItemAttributes
        assert model._nfeatures == side.nfeatures and all(
            sorted(side.public_features[f] for f in set(side.feature_map[data.private_items[i]])) == model._item_features[i]
            for i in range(data.num_items))
    model.train()
    assert len(model._losses) == 2 and np.isfinite(model._losses).all()
    assert model._losses[1] * 2 < model._losses[0] * 1                             # sum / (epoch + 1): the second epoch's sum is lower
    want, decided = dense_lists(model, data)
    recs = model.get_recommendations(K)[1]
    got = np.array([[data.public_items[i] for i, _ in recs[data.private_users[u]]] for u in range(data.num_users)])
    assert decided.sum() > data.num_users // 2 and np.array_equal(got[decided], want[decided])
    path = str(tmp_path / "fm.pkl")
    model._model.save_weights(path)
    other = FM(data=data, config=cfg, params=params(seed=7))
    assert not torch.equal(other._model.state.E, model._model.state.E)
    other._model.load_weights(path)
    mask = model.get_candidate_mask()
    a, b = model._model.recommend(mask, K, 0, data.num_users), other._model.recommend(mask, K, 0, data.num_users)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and other._model.state.step == model._model.state.step


def test_the_replay_sampler_is_refused(ctx, tmp_path):
    from elliot_amd.recommender import FM
    data, cfg = experiment(tmp_path)
    with pytest.raises(Exception, match="replay"):
        FM(data=data, config=cfg, params=params(sampler="replay"))
