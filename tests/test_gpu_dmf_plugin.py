"""GPU end-to-end: the DMF plugin (recommender/neural/DMF) on the ratings of config_files/attribute_sample/: the sample config through
run_experiment, two epochs through RecMixin.train() / evaluate(), one seed repeats bit for bit and two seeds differ, a checkpoint round
trip gives the same top-10."""
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
    base = dict(seed=42, epochs=2, batch_size=64, lr=0.01, reg=0.001, user_mlp="(16,8)", item_mlp="(8,)", neg_ratio=2, similarity="cosine")
    return SimpleNamespace(meta=SimpleNamespace(verbose=False), **{**base, **kw})


def test_the_sample_config_runs(ctx, tmp_path, monkeypatch):
    from elliot_amd import run as runner
    monkeypatch.chdir(tmp_path)
    runner.run_experiment(os.path.join(REPO, "config_files", "sample_dmf_amd.yml"))


@pytest.mark.parametrize("axis", ["reference", "row"])
def test_seeds_and_a_checkpoint_round_trip(ctx, tmp_path, axis):
    from elliot_amd import external, recommender
    assert external.DMF is recommender.DMF and "DMF" in recommender.__all__
    data, cfg = sample_experiment.experiment(tmp_path, K)
    models = [recommender.DMF(data=data, config=cfg, params=params(seed=s, cosine_axis=axis)) for s in (42, 42, 7)]
    for m in models:
        m.train()
    a, b, c = (m._model.state for m in models)
    assert models[0].name.startswith("DMF_") and len(models[0]._losses) == 2 and np.isfinite(models[0]._losses).all()
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in a.names) and not torch.equal(a.uW0, c.uW0)
    recs = models[0].get_recommendations(K)[1]
    assert all(len(recs[data.private_users[u]]) == K for u in range(data.num_users))
    path = str(tmp_path / "dmf.pkl")
    models[0]._model.save_weights(path)
    models[2]._model.load_weights(path)
    mask = models[0].get_candidate_mask()
    x, y = (m._model.recommend(mask, K, 0, min(64, data.num_users)) for m in (models[0], models[2]))
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and c.step == a.step
