"""GPU end-to-end: the BPRSlim plugin through RecMixin on the golden cases (tests/golden/bprslim_ref.npz, written by
scripts/gen_golden_bprslim.py from the reference's own BPRSlimModel and sampler) -- the replayed triplets, S after every epoch, the
loss handed to evaluate(), the lists, scoring from a restored S, checkpoints in both directions, the batch size, the name, the
memory guard and the mini runner on the sample configuration.

Parity bound of a trained S: max(4 d_reorder, 1e-12), d_reorder the reference's own sensitivity to the order of its chain as the
generator measured it (the reference against its math.fsum twin): the shape of a triplet's sum is all that differs."""
import os
import pickle
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd.dataset.dataset import DataSet, default_config
from tests.helpers import bprslim_ref as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UOFF, IOFF = 1000, 5000                       # public ids differ from private ones
U53 = 2.0 ** -53
_pred = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def params(g=None, tag=None, **kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    hyper = br.hyper(g, tag) if g is not None else {}
    return SimpleNamespace(meta=meta, **{"epochs": 2, "seed": 42, "batch_size": 1, **hyper, **kw})


def config(tmp_path):
    cfg = default_config(top_k=10, cutoffs=[10, 5], simple_metrics=["nDCG", "Recall"], out_dir=str(tmp_path))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    return cfg


def fixture_data(tmp_path, g, tag):
    """The case's dict-order rows as the train file of a DataSet (public ids = fixture ids + offsets, every fixture id known
    to it, so an item nobody rated keeps its row), one unseen test item per user."""
    indptr, indices, U, I = br.case(g, tag)
    users = np.repeat(np.arange(U), np.diff(indptr))
    rs = np.random.RandomState(1)
    te_i = [rs.choice(np.setdiff1d(np.arange(I), indices[indptr[u]:indptr[u + 1]])) for u in range(U)]
    cfg = config(tmp_path)
    tr = (users + UOFF, indices.astype(np.int64) + IOFF, g[f"{tag}_ratings"])
    te = (np.arange(U) + UOFF, np.asarray(te_i) + IOFF, np.ones(U))
    data = DataSet(cfg, tr, te, public_users=np.arange(U) + UOFF, public_items=np.arange(I) + IOFF)
    assert (data.num_users, data.num_items, data.transactions) == (U, I, len(indices))
    return data, cfg


def unmasked_predictions(g, tag):
    """(pred [U, I], allowed [U, I]) of a case's last S from the restatement: computed once, shared, never written to."""
    if tag not in _pred:
        indptr, indices, U, I = br.case(g, tag)
        allowed = np.ones((U, I), dtype=bool)
        allowed[np.repeat(np.arange(U), np.diff(indptr)), indices] = False
        _pred[tag] = br.predictions(*br.sorted_rows(indptr, indices), g[f"{tag}_S"][-1]), allowed
    return _pred[tag]


@pytest.mark.parametrize("tag", br.CASES)
def test_plugin_reproduces_the_reference_run(ctx, golden, tmp_path, tag):
    from elliot_amd.recommender import BPRSlim
    g = golden("bprslim_ref.npz")
    data, cfg = fixture_data(tmp_path, g, tag)
    model = BPRSlim(data=data, config=cfg, params=params(g, tag, sampler="replay"))
    st = model._model.state
    assert not st.S.any().item() and st.S.dtype == torch.float64
    seen, snaps, losses = [], [], []
    train_step, evaluate = model._model.train_step, model.evaluate

    def spy_step(batch):
        seen.append(np.stack([x.cpu().numpy().reshape(-1) for x in batch]))
        return train_step(batch)

    def spy_evaluate(it, loss):
        snaps.append(st.S.cpu().numpy())
        losses.append((it, loss))
        return evaluate(it, loss)
    model._model.train_step, model.evaluate = spy_step, spy_evaluate
    ctx.timing(True)
    try:
        model.train()
        kernels = set(ctx.timing_report())
    finally:
        ctx.timing(False)
    assert {"k_bprslim_apply", "k_bprslim_table", "k_bprslim_scores"} <= kernels
    assert len(seen) == len(snaps) == 2 and len(model._results) == 2
    bound = max(4 * float(g[f"{tag}_d_reorder"]), 1e-12)
    indptr, indices, U, I = br.case(g, tag)
    lens = np.diff(indptr)
    for e in range(2):
        trip, S_ref, x_ref = g[f"{tag}_trip"][e], g[f"{tag}_S"][e], g[f"{tag}_x"][e]
        assert np.array_equal(seen[e], trip)                                  # the reference's own triplets
        err = float(np.abs(snaps[e] - S_ref).max())
        print(f"{tag} epoch {e + 1}: max |S - reference| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (tag, e, err)
        assert not np.diag(snaps[e]).any()
        # the loss: x_t sums len_t differences of cells that are each within `bound` of the reference's, and the tree and the
        # chain are each within gamma_{len+1} (2 len max|S|) of the exact sum; a step moves a cell by at most lr (g <= 1 and
        # the decay shrinks it), so max|S| <= lr * (steps so far); |x'^2 - x^2| <= d (2 |x| + d); the n additions of the
        # squares cost gamma_n of their sum
        L = lens[trip[0]].astype(np.float64)
        n = trip.shape[1]
        smax = br.hyper(g, tag)["lr"] * n * (e + 1)
        d = 2 * L * bound + 2 * ((L + 1) * U53 / (1 - (L + 1) * U53)) * 2 * L * smax
        tol = (float(np.sum(d * (2 * np.abs(x_ref) + d))) + 2 * n * U53 * float(np.sum(x_ref ** 2))) / (e + 1)
        it, loss = losses[e]
        want = float(g[f"{tag}_loss"][e]) / (e + 1)                           # evaluate(it, loss / (it + 1)), bprslim.py:117
        print(f"{tag} epoch {e + 1}: loss {loss!r}, reference {want!r}, |difference| {abs(loss - want):.3e} (bound {tol:.3e})")
        assert it == e and abs(loss - want) <= tol
    assert 0.0 <= model.get_results()[10]["test_results"]["nDCG"] <= 1.0
    # lists: every user outside the golden file's `fragile` flag has the reference's ten ids
    recs = model.get_recommendations(10)[1]
    fragile, ref_idx = g[f"{tag}_fragile"], g[f"{tag}_rec_idx"]
    compared = 0
    for u in range(U):
        if fragile[u]:
            continue
        n_ref = int((ref_idx[u] >= 0).sum())
        assert [item - IOFF for item, _ in recs[u + UOFF]] == ref_idx[u, :n_ref].tolist(), u
        compared += 1
    assert compared >= 0.95 * U


@pytest.mark.parametrize("tag", ["plain", "short_rows"])
def test_scoring_from_the_reference_s_matrix(ctx, golden, tmp_path, tag):
    """The reference's pickle ({'_s_dense': S}, written from the golden S) restored: every user's value list equals the
    reference's bit for bit, the ids wherever the value is unique among the user's unmasked predictions."""
    from elliot_amd.recommender import BPRSlim
    g = golden("bprslim_ref.npz")
    data, cfg = fixture_data(tmp_path, g, tag)
    model = BPRSlim(data=data, config=cfg, params=params(g, tag, meta={"restore": True}))
    os.makedirs(os.path.dirname(model._saving_filepath), exist_ok=True)
    with open(model._saving_filepath, "wb") as f:
        pickle.dump({"_s_dense": g[f"{tag}_S"][-1]}, f)
    model.train()
    assert len(model._results) == 1
    recs = model.get_recommendations(10)[1]
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


def test_our_checkpoint_is_the_reference_s_pickle(ctx, golden, tmp_path):
    from elliot_amd.recommender import BPRSlim
    g = golden("bprslim_ref.npz")
    data, cfg = fixture_data(tmp_path, g, "plain")
    model = BPRSlim(data=data, config=cfg, params=params(g, "plain", sampler="replay", meta={"save_weights": True}))
    model.train()
    with open(model._saving_filepath, "rb") as f:
        state = pickle.load(f)                                                # what the reference's set_model_state takes as it is
    assert list(state) == ["_s_dense"] and isinstance(state["_s_dense"], np.ndarray)
    assert state["_s_dense"].dtype == np.float64 and state["_s_dense"].shape == (data.num_items, data.num_items)
    best = model.get_best_arg()
    assert np.abs(state["_s_dense"] - g["plain_S"][best]).max() <= max(4 * float(g["plain_d_reorder"]), 1e-12)
    again = BPRSlim(data=data, config=cfg, params=params(g, "plain", meta={"restore": True}))
    assert not again._model.state.S.any().item()
    again.train()
    assert np.array_equal(bits(again._model.state.S.cpu().numpy()), bits(state["_s_dense"]))
    with pytest.raises(Exception, match="shape"):
        again._model.set_model_state({"_s_dense": np.zeros((3, 3))})


def test_batch_size_cannot_change_the_result(ctx, golden, tmp_path):
    from elliot_amd.recommender import BPRSlim
    g = golden("bprslim_ref.npz")
    data, cfg = fixture_data(tmp_path, g, "plain")
    out = {}
    for bs in (1, 7, 512):
        model = BPRSlim(data=data, config=cfg, params=params(g, "plain", batch_size=bs, epochs=1))
        model.train()
        out[bs] = bits(model._model.state.S.cpu().numpy())
    assert out[1].any() and np.array_equal(out[1], out[7]) and np.array_equal(out[1], out[512])


def test_name_shortcuts_and_defaults(ctx, golden, tmp_path):
    from elliot_amd.recommender import BPRSlim
    g = golden("bprslim_ref.npz")
    data, cfg = fixture_data(tmp_path, g, "defaults")
    model = BPRSlim(data=data, config=cfg, params=params(epochs=3, batch_size=512))
    assert (model._lr, model._lj_reg, model._li_reg) == (0.001, 0.001, 0.1)
    assert model.name == "BPRSlim_seed=42_e=3_bs=512_lr=0$001_ljreg=0$001_lireg=0$1"
    st = model._model.state
    assert (st.lr, st.lj_reg, st.li_reg) == (0.001, 0.001, 0.1) and model._sampler.philox
    model = BPRSlim(data=data, config=cfg, params=params(g, "plain", batch_size=-1))
    assert model._batch_size == data.transactions                             # bprslim.py:63-64
    assert model.name == f"BPRSlim_seed=42_e=2_bs={data.transactions}_lr=0$05_ljreg=0$001_lireg=0$1"
    with pytest.raises(ValueError, match="sampler"):
        BPRSlim(data=data, config=cfg, params=params(sampler="mt"))


def test_memory_guard_refuses_before_allocation(ctx, golden, tmp_path, monkeypatch):
    from elliot_amd import ops
    from elliot_amd.recommender import BPRSlim
    g = golden("bprslim_ref.npz")
    data, cfg = fixture_data(tmp_path, g, "plain")
    need = ops.bprslim_memory_need(data.num_items, data.num_users)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(ctx.device)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, 1 << 40))
    with pytest.raises(ValueError, match=f"{data.num_items} items need {need} bytes of device memory .* {need - 1} bytes are free"):
        BPRSlim(data=data, config=cfg, params=params())
    assert torch.cuda.memory_allocated(ctx.device) == before
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need, 1 << 40))
    BPRSlim(data=data, config=cfg, params=params())                           # exactly enough is enough


def test_mini_runner_on_the_sample_configuration(ctx, tmp_path):
    """The shipped yml beside the shipped sample data, copied as they are; only the output folders are added."""
    import yaml
    from elliot_amd.run import run_experiment
    shutil.copytree(os.path.join(ROOT, "config_files", "attribute_sample"), tmp_path / "config_files" / "attribute_sample")
    with open(os.path.join(ROOT, "config_files", "sample_bprslim_amd.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert not any(k.startswith("path_output") for k in cfg["experiment"])
    cfg["experiment"].update(path_output_rec_result="../out/recs/", path_output_rec_weight="../out/weights/",
                             path_output_rec_performance="../out/perf/")
    with open(tmp_path / "config_files" / "sample_bprslim_amd.yml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    res = run_experiment(str(tmp_path / "config_files" / "sample_bprslim_amd.yml"))
    assert list(res) == ["BPRSlim_seed=42_e=3_bs=512_lr=0$05_ljreg=0$001_lireg=0$1"]
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["nDCG"] <= 1.0
    assert sorted(os.listdir(tmp_path / "out" / "recs")) == sorted(f"{n}_it={e}.tsv" for n in res for e in (1, 2, 3))
