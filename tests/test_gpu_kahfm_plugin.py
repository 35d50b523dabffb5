"""GPU end-to-end: the KaHFM plug-in on the two golden cases (tests/golden/kahfm_ref*.npz, scripts/gen_golden_kahfm.py) with the
reference's replayed triplets, through RecMixin, from the reference's checkpoint, and through the mini runner on the sample
configuration.

Parity bound: max(4 d_reorder, 1e-12), d_reorder the reference's own sensitivity to the order of its dot product as the generator
measured it (the reference run against its math.fsum twin); 1e-12 is the bound of the BPRMF golden test, whose kernel the narrow
case goes through."""
import os
import pickle
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

from tests.helpers import kahfm_ref as kr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden, tmp_path_factory):
    z = golden("kahfm_ref.npz")
    folder = tmp_path_factory.mktemp("kahfm")
    return {tag: kr.load(z, tag, folder) for tag in kr.CASES}


def params(z, **kw):
    meta = SimpleNamespace(**{"verbose": False, **kw.pop("meta", {})})
    hyper = {k[len("hyper_"):]: float(z[k]) for k in z.files if k.startswith("hyper_")}
    hyper = {k: int(v) if v == int(v) else v for k, v in hyper.items()}           # `bias_regularization: 0` prints as 0 in the name
    return SimpleNamespace(meta=meta, epochs=2, seed=42, **{**hyper, **kw})


def trained_tables(golden, z, tag, epoch):
    src = golden(f"kahfm_ref_{tag}_e{epoch}.npz") if tag == "wide" else z
    return tuple(src[f"{tag}_{name}_e{epoch}"] for name in ("P", "Q", "b"))


def reference_lists(fx):
    z, tag, data = fx.z, fx.tag, fx.data
    return {data.private_users[u]: [data.private_items[i] for i in z[f"{tag}_rec_idx"][u].tolist()] for u in range(data.num_users)}


def items_of(recs):
    return {u: [i for i, _ in lst] for u, lst in recs.items()}


@pytest.mark.parametrize("tag", kr.CASES)
def test_plugin_reproduces_the_reference_run(ctx, golden, cases, tag):
    from elliot_amd.recommender import KaHFM
    fx, z = cases[tag], cases[tag].z
    model = KaHFM(data=fx.data, config=fx.cfg, params=params(z, sampler="replay"))
    assert model.name == str(z[f"{tag}_name"]) and model.name.startswith("KaHFM") and model._batch_size == 10000
    assert model._embed_k == z[f"{tag}_features"].shape[0] == model._model.state.F
    st = model._model.state
    assert kr.same_bits(st.P.cpu().numpy(), z[f"{tag}_P0"]) and kr.same_bits(st.Q.cpu().numpy(), z[f"{tag}_Q0"])
    seen, snaps = [], []
    train_step, evaluate = model._model.train_step, model.evaluate

    def spy_step(batch, **kw):
        seen.append(np.stack([x.cpu().numpy().reshape(-1) for x in batch]))
        return train_step(batch, **kw)

    def spy_evaluate(*a, **kw):
        assert len(a) == 1 and not kw                                             # no loss is passed to evaluate
        snaps.append(tuple(getattr(st, name).cpu().numpy() for name in ("P", "Q", "b")))
        return evaluate(*a, **kw)
    model._model.train_step, model.evaluate = spy_step, spy_evaluate
    ctx.timing(True)
    try:
        model.train()
        kernels = set(ctx.timing_report())
    finally:
        ctx.timing(False)
    assert ("k_bprsgd_apply_wide" in kernels) == (tag == "wide") and ("k_bprsgd_apply" in kernels) == (tag == "narrow")
    assert len(seen) == len(snaps) == 2
    bound = max(4 * float(z[f"{tag}_d_reorder"]), 1e-12)
    for e in range(2):
        assert np.array_equal(seen[e], z[f"{tag}_trip"][e])                       # the reference's own triplets
        for name, got, ref in zip("PQb", snaps[e], trained_tables(golden, z, tag, e + 1)):
            err = np.abs(got - ref).max()
            print(f"{tag} epoch {e + 1} {name}: max |ours - reference| {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (tag, e, name, err)
    assert 0.0 < model.get_results()[10]["test_results"]["nDCG"] <= 1.0
    recs = model.get_recommendations(10)[1]
    assert items_of(recs) == reference_lists(fx)
    vals = np.array([[s for _, s in recs[fx.data.private_users[u]]] for u in range(fx.data.num_users)])
    # a score is b + p.q: parameters within `bound` move it by at most bound (1 + sum|p| + sum|q|), its own summation order by
    # at most gamma_F sum|p||q|
    P, Q, _ = snaps[1]
    F = P.shape[1]
    tol = bound * (1 + np.abs(P).sum(axis=1).max() + np.abs(Q).sum(axis=1).max()) + \
        2 * F * 2.0 ** -53 * (np.abs(P).max(axis=0) * np.abs(Q).max(axis=0)).sum()
    assert np.abs(vals - z[f"{tag}_rec_val"]).max() <= tol


def test_reference_checkpoint_restores(ctx, cases):
    """KAHFMModel.save_weights' pickle (the narrow case after its second epoch): loaded by `restore`, evaluated, the same lists;
    our checkpoint has the same four keys, shapes and types."""
    from elliot_amd.recommender import KaHFM
    fx = cases["narrow"]
    model = KaHFM(data=fx.data, config=fx.cfg, params=params(fx.z, meta={"restore": True}))
    shutil.copyfile(os.path.join(kr.GOLDEN, "kahfm_ref_weights.pkl"), model._saving_filepath)
    model.train()
    assert 0.0 < model.get_results()[10]["test_results"]["nDCG"] <= 1.0
    assert items_of(model.get_recommendations(10)[1]) == reference_lists(fx)
    with open(model._saving_filepath, "rb") as fh:
        theirs = pickle.load(fh)
    ours = model._model.get_model_state()
    assert set(ours) == set(theirs) == {"_user_bias", "_item_bias", "_user_factors", "_item_factors"}
    for key in theirs:
        assert ours[key].shape == theirs[key].shape and ours[key].dtype == theirs[key].dtype
        assert np.array_equal(ours[key], theirs[key])


def test_item_attributes_serve_as_the_loader_too(ctx, golden, tmp_path):
    """`loader: ItemAttributes`: the reference only reads feature_map / features / public_features of the namespace."""
    from elliot_amd.recommender import KaHFM
    from tests.helpers import attr_fixture as fxm
    fx = fxm.load(golden("attr_ref.npz"), tmp_path)
    model = KaHFM(data=fx.data, config=fx.cfg, params=SimpleNamespace(meta=SimpleNamespace(verbose=False), epochs=1, loader="ItemAttributes"))
    assert model.name.endswith("load=ItemAttributes") and model._embed_k == fx.data.side_information.ItemAttributes.nfeatures
    P0, Q0 = kr.start_tables(fx.data, fx.data.side_information.ItemAttributes)
    assert kr.same_bits(model._model.state.P.cpu().numpy(), P0) and kr.same_bits(model._model.state.Q.cpu().numpy(), Q0)
    model.train()
    assert 0.0 < model.get_results()[10]["test_results"]["nDCG"] <= 1.0


def test_external_entry_point_resolves():
    import elliot_amd.external as external
    from elliot_amd import recommender as rec
    assert external.KaHFM is rec.KaHFM and "KaHFM" in rec.__all__


def test_mini_runner_on_the_sample_configuration(ctx, tmp_path):
    """The shipped yml beside the shipped sample data, copied as they are; only the output folders are added."""
    import yaml
    from elliot_amd.run import run_experiment
    for folder in ("attribute_sample", "kg_sample"):
        shutil.copytree(os.path.join(ROOT, "config_files", folder), tmp_path / "config_files" / folder)
    with open(os.path.join(ROOT, "config_files", "sample_kahfm_amd.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert not any(k.startswith("path_output") for k in cfg["experiment"])
    cfg["experiment"].update(path_output_rec_result="../out/recs/", path_output_rec_weight="../out/weights/",
                             path_output_rec_performance="../out/perf/")
    with open(tmp_path / "config_files" / "sample_kahfm_amd.yml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    res = run_experiment(str(tmp_path / "config_files" / "sample_kahfm_amd.yml"))
    assert list(res) == ["KaHFM_seed=42_e=2_bs=10000_lr=0$05_b_reg=0_u_reg=0$0025_pos_i_reg=0$0025_neg_it_reg=0$00025_load=ChainedKG"]
    for r in res.values():
        assert 0.0 < r[10]["test_results"]["nDCG"] <= 1.0
    assert sorted(os.listdir(tmp_path / "out" / "recs")) == sorted(f"{n}_it={e}.tsv" for n in res for e in (1, 2))     # one per epoch
