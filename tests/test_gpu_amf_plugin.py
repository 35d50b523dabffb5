"""GPU end-to-end: the AMF plugin (recommender/adversarial/AMF) on the toy data of test_gpu_rank_plugin (200 x 300).

The training comparison uses the tolerance of tests/test_gpu_amf.py: per compared array 4 x the distance between the float32 and
the float64 run of the restatement (tests/helpers/amf_ref.py) fed the same triplets, floored at one float32 ulp; the ratios are
printed before the assertion (measured on an MI355X after 4 epochs, 2 of them adversarial: 0.23 - 0.25 of the bound for Bi, Gu, Gi,
dGu, dGi).  Everything else here is exact.
"""
import os
import pickle
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd import ops
from tests.helpers import amf_ref
from tests.test_gpu_rank_plugin import experiment

pytestmark = pytest.mark.gpu

BASE = dict(batch_size=512, factors=16, lr=0.01, l_w=0.1, l_b=0.001)


def params(meta=None, **kw):
    return SimpleNamespace(meta=SimpleNamespace(verbose=False, **(meta or {})), seed=42, **{**BASE, **kw})


def test_without_adversarial_epochs_amf_is_bprmf_batch_bit_for_bit(ctx, tmp_path, lib_option):
    """The comparison needs a BPRMF_batch whose own bits repeat from run to run.  With the dense accumulators of a small model its
    step adds gradient rows with float atomics in two places: everywhere on the path of batches under 2048 triplets, and, on the
    sorted path, for a user segment that a chunk boundary cuts.  So: one batch per epoch (batch_size -1 = all `transactions`
    samples, >= 2048: the sorted path) and one user chunk over the whole batch (`uchunk`: no user segment is cut).  The item side
    of the sorted path sums in a fixed order as it is."""
    from elliot_amd.recommender import AMF, BPRMF_batch
    data, cfg = experiment(tmp_path, False, metrics=["nDCG"], gate=False)
    assert 2048 <= data.transactions <= 8192
    lib_option("uchunk", 8192)
    a = AMF(data=data, config=cfg, params=params(epochs=2, adversarial_epochs=0, eps=0.5, l_adv=1.0, batch_size=-1))
    b = BPRMF_batch(data=data, config=cfg, params=params(epochs=2, batch_size=-1))
    a.train(), b.train()
    sa, sb = a._model.state, b._model.state
    assert sa.step == sb.step > 0
    for n in ("Gu", "Gi", "Bi", "mGu", "vGu", "mGi", "vGi", "mBi", "vBi"):
        assert torch.equal(getattr(sa, n), getattr(sb, n)), n
    assert a._model.amf.delta_is_zero and not a._model.amf.dGu.any()


def test_four_epochs_two_of_them_adversarial_against_the_restatement(ctx, tmp_path):
    from elliot_amd.recommender import AMF
    data, cfg = experiment(tmp_path, False, metrics=["nDCG"], gate=False)
    p = params(epochs=4, adversarial_epochs=2, eps=0.5, l_adv=1.0)
    model = AMF(data=data, config=cfg, params=p)
    st = model._model.state
    start = [st.Gu.cpu().numpy().copy(), st.Gi.cpu().numpy().copy(), st.Bi.cpu().numpy().copy()]
    refs = [amf_ref.Model(*start, p.l_w, p.l_b, p.eps, p.l_adv, dt) for dt in (torch.float64, torch.float32)]
    for it in range(p.epochs):
        adv = (p.epochs - it) <= p.adversarial_epochs
        for batch in model._sampler.step(data.transactions, p.batch_size):
            model._model.train_step(batch, adv)
            host = tuple(t.cpu().numpy() for t in batch)
            for r in refs:
                r.train_step(host, adv, p.lr)
    assert st.step == refs[0].step == 4 * -(-data.transactions // p.batch_size)
    amf = model._model.amf
    got = [st.Bi, st.Gu, st.Gi, amf.dGu, amf.dGi]
    want = [[r.Bi, r.Gu, r.Gi, r.dGu, r.dGi] for r in refs]
    bad = []
    for k, (g, a, b) in enumerate(zip(got, *want)):
        tol, dist = amf_ref.bound(a.numpy(), b.numpy()), amf_ref.distance(g.cpu().numpy(), a.numpy())
        print(f"array {k}: |device - f64| = {dist:.3e}, bound {tol:.3e}, ratio {dist / tol:.3f}")
        if not dist <= tol:
            bad.append((k, dist, tol))
    assert not bad, bad
    assert not amf.delta_is_zero and amf.dGu.any()


def test_eval_perturbations_write_the_references_table_and_leave_delta_set(ctx, tmp_path):
    from elliot_amd.recommender import AMF
    data, cfg = experiment(tmp_path, False, metrics=["nDCG", "Recall"], gate=False)
    model = AMF(data=data, config=cfg, params=params({"eval_perturbations": True}, epochs=2, adversarial_epochs=1, eps=0.5,
                                                     l_adv=1.0, nb_iter=2))
    assert model._eps_iter == 2.5 * 0.5 / 2
    model.train()
    res = model.get_results()
    assert set(res) == {10, 5}
    path = os.path.join(cfg.path_output_rec_performance, f"adversarial-{model.name}.tsv")
    lines = [l.rstrip("\n").split("\t") for l in open(path)]
    assert lines[0] == ["Epoch", "AdvEpoch", "K", "nDCG", "Recall", "SSAP-nDCG", "SSAP-Recall", "MSAP-nDCG", "MSAP-Recall"]
    assert len(lines) == 1 + 2 * 2 and {(r[0], r[1], r[2]) for r in lines[1:]} == {(str(e), "1", str(k)) for e in (0, 1) for k in (10, 5)}
    assert all(0.0 <= float(x) <= 1.0 for r in lines[1:] for x in r[3:])
    amf = model._model.amf
    assert not amf.delta_is_zero and amf.dGu.any() and amf.dGi.any()
    # the perturbation left behind is FGSM's on the full batch: every row has norm eps or is exactly zero
    n = torch.linalg.vector_norm(amf.dGu, dim=1).cpu().numpy()
    assert (np.isclose(n, 0.5, rtol=1e-5) | (n == 0)).all() and (n > 0).any()


def test_adversarial_lists_are_the_top_k_of_the_perturbed_tables(ctx, tmp_path):
    from elliot_amd.recommender import AMF
    data, cfg = experiment(tmp_path, False, metrics=["nDCG"], gate=False)
    model = AMF(data=data, config=cfg, params=params(epochs=1, adversarial_epochs=1, eps=0.5, l_adv=1.0))
    model.train()
    m, mask = model._model, model.get_candidate_mask()
    idx, val = m.recommend(mask, 10, 0, data.num_users, adversarial=True)
    Pu, Pi = m.amf.perturbed_tables()
    assert torch.equal(Pu, m.state.Gu + m.amf.dGu) and torch.equal(Pi, m.state.Gi + m.amf.dGi)
    widx, wval = ops.score_topk(ctx, Pu, Pi, m.state.Bi, 0, data.num_users, 10, excl=mask[1])
    assert torch.equal(idx, widx) and torch.equal(val, wval)
    cidx, _ = m.recommend(mask, 10, 0, data.num_users)
    assert not torch.equal(cidx, idx)                              # eps = 0.5 moves the lists
    recs = model.get_recommendations(10, adversarial=True)[1]
    u0 = data.private_users[0]
    assert [i for i, _ in recs[u0]] == [data.private_items[int(x)] for x in idx[0].cpu().tolist()]


def test_checkpoint_round_trips_delta_and_the_step_counter(ctx, tmp_path):
    from elliot_amd.recommender import AMF
    data, cfg = experiment(tmp_path, False, metrics=["nDCG"], gate=False)
    p = params(epochs=2, adversarial_epochs=1, eps=0.5, l_adv=1.0)
    model = AMF(data=data, config=cfg, params=p)
    model.train()
    path = str(tmp_path / "amf.pkl")
    model._model.save_weights(path)
    keys = set(pickle.load(open(path, "rb")))
    assert keys >= {"_user_factors", "_item_factors", "_item_bias", "_step", "mGu", "vGu", "mGi", "vGi", "mBi", "vBi", "_delta_Gu", "_delta_Gi"}
    other = AMF(data=data, config=cfg, params=p)
    other._model.load_weights(path)
    a, b = model._model, other._model
    assert b.state.step == a.state.step > 0 and not b.amf.delta_is_zero
    for x, y in ((a.amf.dGu, b.amf.dGu), (a.amf.dGi, b.amf.dGi), (a.state.Gu, b.state.Gu), (a.state.vGi, b.state.vGi)):
        assert torch.equal(x, y)
    # the restored row lists clear exactly the non-zero rows, and the two models take the same next step
    batch = next(iter(model._sampler.step(512, 512)))
    a.train_step(batch, True), b.train_step(batch, True)
    assert torch.equal(a.state.Gu, b.state.Gu) and torch.equal(a.amf.dGi, b.amf.dGi) and torch.equal(a.state.Bi, b.state.Bi)


def test_more_adversarial_epochs_than_epochs_raise_the_references_message(ctx, tmp_path):
    from elliot_amd.recommender import AMF
    data, cfg = experiment(tmp_path, False, metrics=["nDCG"], gate=False)
    with pytest.raises(Exception, match=r"The total epoch \(2\) is smaller than the adversarial epochs \(3\)\."):
        AMF(data=data, config=cfg, params=params(epochs=2, adversarial_epochs=3))
    assert AMF(data=data, config=cfg, params=params(epochs=5))._adversarial_epochs == 2      # default: epochs // 2


def test_auc_is_reported_with_rank_metrics(ctx, tmp_path):
    from elliot_amd.recommender import AMF
    data, cfg = experiment(tmp_path, False)
    model = AMF(data=data, config=cfg, params=params(epochs=2, adversarial_epochs=1, eps=0.5, l_adv=1.0))
    model.train()
    got = model.get_results()[10]["test_results"]
    assert list(got) == ["nDCG", "AUC", "GAUC", "LAUC"] and 0.0 < got["AUC"] < 1.0


def test_external_amf_resolves(ctx):
    import importlib.util
    import elliot_amd.external as ext
    spec = importlib.util.spec_from_file_location("external", ext.__file__)
    module = importlib.util.module_from_spec(spec)
    saved = sys.modules.get("external")
    sys.modules["external"] = module
    try:
        spec.loader.exec_module(module)
        assert getattr(module, "AMF").__name__ == "AMF"
    finally:
        if saved is None:
            del sys.modules["external"]
        else:
            sys.modules["external"] = saved
