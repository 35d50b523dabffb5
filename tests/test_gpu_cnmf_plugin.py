"""GPU end-to-end: the ConvNeuMF plugin (recommender/neural/ConvNeuMF) on the ratings of config_files/attribute_sample/: the sample
config through run_experiment, two epochs through RecMixin.train() / evaluate(), one seed repeats bit for bit and two seeds differ,
every user gets K recommendations, a checkpoint round trip gives the same top-10."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import sample_experiment

pytestmark = pytest.mark.gpu

K = 10
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(**kw):
    base = dict(seed=42, epochs=2, batch_size=64, lr=0.005, l_w=0.005, l_b=0.0005, embedding_size=9, cnn_channels="(1, 5, 3)",
                cnn_kernels="(2,2)", cnn_strides="(2,2)", dropout_prob=0.2)
    return SimpleNamespace(meta=SimpleNamespace(verbose=False), **{**base, **kw})


def test_the_sample_config_runs(ctx, tmp_path, monkeypatch):
    from elliot_amd import run as runner
    monkeypatch.chdir(tmp_path)
    runner.run_experiment(os.path.join(REPO, "config_files", "sample_convneumf_amd.yml"))


def test_seeds_and_a_checkpoint_round_trip(ctx, tmp_path):
    from elliot_amd import external, recommender
    assert external.ConvNeuMF is recommender.ConvNeuMF and "ConvNeuMF" in recommender.__all__
    data, cfg = sample_experiment.experiment(tmp_path, K)
    models = [recommender.ConvNeuMF(data=data, config=cfg, params=params(seed=s)) for s in (42, 42, 7)]
    for m in models:
        m.train()
    a, b, c = (m._model.state for m in models)
    assert models[0].name.startswith("ConvNeuMF_") and len(models[0]._losses) == 2 and np.isfinite(models[0]._losses).all()
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in a.names) and not torch.equal(a.P, c.P)
    recs = models[0].get_recommendations(K)[1]
    assert all(len(recs[data.private_users[u]]) == K for u in range(data.num_users))
    path = str(tmp_path / "cnmf.pkl")
    models[0]._model.save_weights(path)
    models[2]._model.load_weights(path)
    mask = models[0].get_candidate_mask()
    x, y = (m._model.recommend(mask, K, 0, min(64, data.num_users)) for m in (models[0], models[2]))
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and c.step == a.step
