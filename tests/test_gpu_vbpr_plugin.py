"""GPU end-to-end: the VBPR plugin (recommender/visual_recommenders/VBPR) through RecMixin.train() + evaluate() on a toy data set
(30 users x 50 items) with a tmp-dir feature folder and the replay sampler.

The training comparison uses the tolerance of tests/test_gpu_vbpr.py: per compared array 4 x the distance between the float32 and
the float64 run of the restatement (tests/helpers/vbpr_ref.py) fed the same triplets, floored at one float32 ulp; the ratios are
printed before the assertion (measured on an MI355X after two epochs: 0.18 - 0.28 of the bound for the six variables; all-zero
features against BPRMF_batch 0.05 - 0.12).  The replay sampler's stream does not depend on the model, so a twin sampler hands the restatement
the very triplets the plugin trains on.  Lists are compared on inputs this file checks first: the model seed is chosen ON THE CPU as
the first whose float64 run keeps, for every user, the scores of its candidates down to rank k + 1 more than 100 x the bound apart.
Everything else here is exact.
"""
import os
import pickle
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd import run as runner
from elliot_amd.dataset.samplers import custom_sampler
from elliot_amd.recommender.visual_recommenders.VBPR.VBPR_model import NAMES, initial_weights
from tests.helpers import vbpr_ref

pytestmark = pytest.mark.gpu

NU, NI, D, K = 30, 50, 24, 10
BASE = dict(epochs=2, batch_size=64, batch_eval=16, factors=6, factors_d=4, lr=0.01, l_w=0.01, l_b=0.01, l_e=0.02, sampler="replay")


def params(seed=42, **kw):
    return SimpleNamespace(meta=SimpleNamespace(verbose=False), seed=seed, **{**BASE, **kw})


def experiment(folder, rank_metrics=False, zero_features=False):
    rs = np.random.RandomState(7)
    os.makedirs(folder / "cfg" / "features", exist_ok=True)
    with open(folder / "cfg" / "dataset.tsv", "w") as f:
        for u in range(NU):
            for i in rs.choice(NI, rs.randint(8, 20), replace=False):
                f.write(f"{u + 1}\t{i + 1}\t{rs.randint(1, 6)}\t{rs.randint(0, 10 ** 6)}\n")
    for i in range(NI + 3):                                     # three files belong to items nobody rated
        vec = np.zeros(D, np.float32) if zero_features else np.maximum(rs.standard_normal(D), 0).astype(np.float32)
        np.save(folder / "cfg" / "features" / f"{i + 1}.npy", vec)
    ev = {"simple_metrics": ["nDCG", "AUC", "GAUC", "LAUC"] if rank_metrics else ["nDCG", "Recall"], "cutoffs": [K, 5],
          "relevance_threshold": 3}
    if rank_metrics:
        ev["rank_metrics"] = True
    exp = {"dataset": "toy", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv",
                                             "side_information": [{"dataloader": "VisualAttribute", "visual_features": "features"}]},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": K, "evaluation": ev,
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/"}
    cfg = runner.build_config(exp, str(folder / "cfg"))
    return runner.load_data(exp, cfg, str(folder / "cfg")), cfg


def stream(ctx, data, p):
    """The triplets of p.epochs epochs of the replay sampler: (transactions // batch_size) full batches per epoch, one stream."""
    twin = custom_sampler.Sampler(data.i_train_dict, ctx=ctx, replay=True)
    events = (data.transactions // p.batch_size) * p.batch_size
    out = []
    for _ in range(p.epochs):
        out += [tuple(t.cpu().numpy() for t in batch) for batch in twin.step(events, p.batch_size)]
    assert all(len(b[0]) == p.batch_size for b in out) and len(out) == p.epochs * (data.transactions // p.batch_size)
    return out


def features_of(data):
    side = data.side_information.VisualAttributes
    return side.feature_matrix([data.private_items[i] for i in range(data.num_items)])


def restate(data, p, seed, batches, feat):
    """The float64 and the float32 restatement after the batches, from the plugin's own initial weights."""
    w = initial_weights(seed, data.num_users, data.num_items, p.factors, p.factors_d, feat.shape[1])
    refs = [vbpr_ref.Model(w["Gu"], w["Gi"], w["Bi"], w["Tu"], w["E"], w["Bp"], feat, p.l_w, p.l_b, p.l_e, dt)
            for dt in (torch.float64, torch.float32)]
    for b in batches:
        for r in refs:
            r.train_step(b, p.lr)
    vbpr_ref.check_case(refs)
    return refs


def candidate_scores(data, scores):
    s = np.array(scores, np.float64)
    s[data.sp_i_train.toarray() != 0] = -np.inf                                    # the train items are no candidates
    return s


def separated_seed(data, p, batches, feat):
    for seed in range(42, 42 + 64):
        r64, r32 = restate(data, p, seed, batches, feat)
        p64, p32 = r64.predict_all().numpy(), r32.predict_all().numpy()
        tol = vbpr_ref.bound(p64, p32)
        s = candidate_scores(data, p64)
        order = np.argsort(-s, axis=1, kind="stable")
        top = np.take_along_axis(s, order, axis=1)[:, :K + 2]
        if np.isfinite(top).all() and (np.abs(np.diff(top, axis=1)) > 100 * tol).all():
            return seed, (r64, r32), order[:, :K], tol
    raise AssertionError("no seed separates the scores")


def test_two_epochs_through_recmixin_against_the_restatement_and_a_checkpoint_round_trip(ctx, tmp_path):
    from elliot_amd.recommender import VBPR
    data, cfg = experiment(tmp_path)
    assert data.num_items <= NI and data.side_information.VisualAttributes.visual_features_shape == D
    p = params()
    batches, feat = stream(ctx, data, p), features_of(data)
    seed, (r64, r32), want_lists, tol = separated_seed(data, p, batches, feat)
    p = params(seed=seed)
    model = VBPR(data=data, config=cfg, params=p)
    assert model.name.startswith("VBPR_") and torch.equal(model._model.vb.feat.cpu(), torch.from_numpy(feat))
    model.train()                                                                  # RecMixin.train(): two epochs, evaluate() after each
    res = model.get_results()
    assert set(res) == {K, 5} and 0.0 <= res[K]["test_results"]["nDCG"] <= 1.0 and len(model._results) == 2
    m = model._model
    assert m.state.step == r64.step == len(batches)
    got = m.get_model_state()
    bad = []
    for n in NAMES:
        a, b = getattr(r64, n).numpy(), getattr(r32, n).numpy()
        t, dist = vbpr_ref.bound(a, b), vbpr_ref.distance(got[n].reshape(a.shape), a)
        print(f"{n}: |device - f64| = {dist:.3e}, bound {t:.3e}, ratio {dist / t:.3f}")
        if not dist <= t:
            bad.append((n, dist, t))
    assert not bad, bad
    # the lists, on the separated scores: equal for every user
    idx, val = m.recommend(model.get_candidate_mask(), K, 0, data.num_users)
    assert np.array_equal(idx.cpu().numpy(), want_lists.astype(np.int32))
    recs = model.get_recommendations(K)[1]
    u0 = data.private_users[0]
    assert [i for i, _ in recs[u0]] == [data.private_items[int(x)] for x in want_lists[0]]
    # checkpoint: the reference's six names, and the same lists after a restore into a fresh model
    path = str(tmp_path / "vbpr.pkl")
    m.save_weights(path)
    keys = set(pickle.load(open(path, "rb")))
    assert keys >= set(NAMES) | {"_step"} | {s + n for s in "mv" for n in NAMES}
    other = VBPR(data=data, config=cfg, params=params(seed=seed + 1))
    assert not torch.equal(other._model.state.Gu, m.state.Gu)
    other._model.load_weights(path)
    idx2, val2 = other._model.recommend(other.get_candidate_mask(), K, 0, data.num_users)
    assert torch.equal(idx2, idx) and torch.equal(val2, val) and other._model.state.step == m.state.step
    batch = batches[0]
    m.train_step(batch), other._model.train_step(batch)                            # slots and step counter came along
    assert torch.equal(m.vb.EB, other._model.vb.EB) and torch.equal(m.state.Gi, other._model.state.Gi)


def test_restore_reads_the_saved_weights(ctx, tmp_path):
    from elliot_amd.recommender import VBPR
    data, cfg = experiment(tmp_path)
    p = params(epochs=1)
    p.meta.save_weights = True
    model = VBPR(data=data, config=cfg, params=p)
    model.train()
    q = params(epochs=1)
    q.meta.restore = True
    again = VBPR(data=data, config=cfg, params=q)
    assert again.train() is True
    assert torch.equal(again._model.vb.Tu, model._model.vb.Tu) and again.get_results() == model.get_results()


def test_auc_is_reported_with_rank_metrics(ctx, tmp_path):
    from elliot_amd.recommender import VBPR
    data, cfg = experiment(tmp_path, rank_metrics=True)
    model = VBPR(data=data, config=cfg, params=params())
    model.train()
    got = model.get_results()[K]["test_results"]
    assert list(got) == ["nDCG", "AUC", "GAUC", "LAUC"] and 0.0 < got["AUC"] < 1.0


def test_zero_features_give_bprmf_batchs_tables_within_the_bound(ctx, tmp_path):
    """Not bit for bit: the VBPR kernels walk rows widened by Tu / P (zero products here, but another lane layout and another order
    of the dot products' partial sums than BPRMF_batch's kernels).  Both sides see the same triplets and the same initial Gu, Gi, Bi."""
    from elliot_amd.recommender import BPRMF_batch, VBPR
    data, cfg = experiment(tmp_path, zero_features=True)
    p = params()
    batches, feat = stream(ctx, data, p), features_of(data)
    assert not feat.any()
    model = VBPR(data=data, config=cfg, params=p)
    w = initial_weights(p.seed, data.num_users, data.num_items, p.factors, p.factors_d, D)
    bp = SimpleNamespace(meta=SimpleNamespace(verbose=False), seed=42, epochs=2, batch_size=p.batch_size, factors=p.factors, lr=p.lr,
                         l_w=p.l_w, l_b=p.l_b, sampler="replay")
    plain = BPRMF_batch(data=data, config=cfg, params=bp, init_weights=(w["Gu"], w["Gi"], w["Bi"]))
    for b in batches:
        model._model.train_step(b), plain._model.train_step(b)
    r64, r32 = restate(data, p, p.seed, batches, feat)
    a, b = model._model.state, plain._model.state
    for n in ("Gu", "Gi", "Bi"):
        t = vbpr_ref.bound(getattr(r64, n).numpy(), getattr(r32, n).numpy())
        dist = vbpr_ref.distance(getattr(a, n).cpu().numpy(), getattr(b, n).cpu().numpy())
        print(f"{n}: |VBPR - BPRMF_batch| = {dist:.3e}, bound {t:.3e}, ratio {dist / t:.3f}")
        assert dist <= t, n
    assert a.step == b.step == len(batches)


def test_missing_side_information_and_an_oversized_batch_are_refused(ctx, tmp_path):
    from elliot_amd.recommender import VBPR
    data, cfg = experiment(tmp_path)
    with pytest.raises(Exception, match="VisualAttribute"):
        VBPR(data=data, config=cfg, params=params(loader="Nothing"))
    with pytest.raises(Exception, match="batch_size"):
        VBPR(data=data, config=cfg, params=params(batch_size=10 ** 6))


def test_external_vbpr_resolves(ctx):
    import importlib.util
    import elliot_amd.external as ext
    spec = importlib.util.spec_from_file_location("external", ext.__file__)
    module = importlib.util.module_from_spec(spec)
    saved = sys.modules.get("external")
    sys.modules["external"] = module
    try:
        spec.loader.exec_module(module)
        assert getattr(module, "VBPR").__name__ == "VBPR"
    finally:
        if saved is None:
            del sys.modules["external"]
        else:
            sys.modules["external"] = saved
