"""Generate tests/golden/kahfm_ref*.npz, kahfm_ref_weights.pkl and the input files under tests/golden/kahfm_kg/ by RUNNING THE
REFERENCE'S OWN KaHFM code (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  Loaded BY FILE PATH
under their own dotted names (the loading helpers are those of scripts/gen_golden_attr.py), and run as they are:
  elliot/dataset/modular_loaders/{abstract_loader, kg/kahfm_style, loader_coordinator_mixin}.py
        ChainedKG, LoaderCoordinator.coordinate_information
  elliot/dataset/dataset.py                DataSet.align_with_training, dataframe_to_dict, build_sparse (on a bare instance)
  elliot/dataset/samplers/custom_sampler.py        Sampler
  elliot/recommender/base_recommender_model.py     autoset_params, get_params_shortcut (the `name` string)
  elliot/recommender/knowledge_aware/kaHFM/{tfidf_utils, kahfm_model, kahfm}.py
        TFIDF, KAHFMModel (initialize, train_step, prepare_predictions, get_user_predictions, save_weights), KaHFM.__init__ / name
The other `elliot.*` imports are empty stubs.  RESTATED, as in gen_golden_attr.py: dataset.py:201-217 (the maps of a DataSet) and
KaHFM.train's loop (kahfm.py:161-177: sampler.step(transactions, 10000), model.train_step per batch) without its evaluation.

Inputs are this repository's own synthetic data: small_dataset(80, 120, seed=3) and two knowledge-graph side informations of
small_kg_features (threshold 2): NARROW, 109 Zipf-distributed features of which an odd number below 64 is left, and WIDE, 800
uniformly distributed features of which more than 512 are left.  The split (the last fifth of every user's rows is the test fold)
is this script's own, recorded as flags; the alignment with the training fold reduces the map once more.

Besides the reference run, `d_reorder`: the largest absolute difference of any parameter after either epoch between the
reference run and a run of the subclass below whose indexed_predict sums the dot product with math.fsum, on the same triplets --
the reference's own sensitivity to the order of a sum nobody specifies (BLAS ddot).

The wide case's trained tables go to files of their own (kahfm_ref_wide_e1.npz, kahfm_ref_wide_e2.npz): dense doubles do not
compress, and no committed file may exceed 1 MiB.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_kahfm.py <reference checkout>
"""
import logging
import math
import os
import shutil
import sys
import time
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import pandas as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from gen_golden_attr import real, stub  # noqa: E402
from elliot_amd.synthetic import small_dataset, small_kg_features, write_kg_files  # noqa: E402

K, EPOCHS, THRESHOLD = 10, 2, 2
HYPER = dict(lr=0.05, bias_regularization=0, user_regularization=0.0025, positive_item_regularization=0.0025,
             negative_item_regularization=0.00025)
CASES = {
    "narrow": dict(n_features=109, per_item=(1, 9), zipf=True, missing=(3, 17, 58), extra=(5, 9), seed=11),
    "wide": dict(n_features=800, per_item=(40, 60), zipf=False, missing=(3, 17, 58), extra=(5, 9), seed=12),
}


def load_reference(ref):
    log = SimpleNamespace(get_logger=lambda *a, **k: logging.getLogger("ref"), get_logger_model=lambda *a, **k: logging.getLogger("ref"))
    stub("elliot.utils", logging=log)
    stub("elliot.utils.folder", build_model_folder=None)
    stub("elliot.utils.write", store_recommendation=None)
    stub("elliot.evaluation.evaluator", Evaluator=object)
    stub("elliot.recommender.early_stopping", EarlyStopping=object)
    stub("elliot.recommender.recommender_utils_mixin", RecMixin=type("RecMixin", (), {k: None for k in ("get_loss", "get_params", "get_results")}))
    stub("elliot.splitter.base_splitter", Splitter=object)
    stub("elliot.prefiltering.standard_prefilters", PreFilter=object)
    stub("elliot.negative_sampling.negative_sampling", NegativeSampler=object)
    m = SimpleNamespace()
    real(ref, "elliot.dataset.modular_loaders.abstract_loader")
    m.kahfm_style = real(ref, "elliot.dataset.modular_loaders.kg.kahfm_style")
    stub("elliot.dataset.modular_loaders.loaders", ChainedKG=m.kahfm_style.ChainedKG)
    m.coordinator = real(ref, "elliot.dataset.modular_loaders.loader_coordinator_mixin")
    real(ref, "elliot.dataset.abstract_dataset")
    m.dataset = real(ref, "elliot.dataset.dataset")
    m.sampler = real(ref, "elliot.dataset.samplers.custom_sampler")
    stub("elliot.dataset.samplers", custom_sampler=m.sampler)
    m.base = real(ref, "elliot.recommender.base_recommender_model")
    m.base.init_charger = lambda init: init
    pkg = "elliot.recommender.knowledge_aware.kaHFM"
    m.tfidf = real(ref, f"{pkg}.tfidf_utils")
    m.model = real(ref, f"{pkg}.kahfm_model")
    m.plugin = real(ref, f"{pkg}.kahfm")
    return m


def map_fields(out, tag, fmap):
    out[f"{tag}_item"] = np.asarray(list(fmap.keys()), np.int64)
    out[f"{tag}_indptr"] = np.concatenate([[0], np.cumsum([len(v) for v in fmap.values()])]).astype(np.int64)
    out[f"{tag}_feat"] = np.asarray([f for v in fmap.values() for f in v], np.int64)


def run_case(m, tag, frame, folder, out, big):
    log = logging.getLogger("ref")
    side_cfg = SimpleNamespace(dataloader="ChainedKG", map=os.path.join(folder, "map.tsv"), features=os.path.join(folder, "features.tsv"),
                               properties=os.path.join(folder, "properties.conf"), additive=True, threshold=THRESHOLD)
    clean, side = m.coordinator.LoaderCoordinator().coordinate_information(frame, sides=[side_cfg], logger=log)
    out[f"{tag}_coord_items"] = np.sort(np.asarray(list(side.ChainedKG.object.get_mapped()[1]), np.int64))
    out[f"{tag}_coord_features"] = np.asarray(side.ChainedKG.features, np.int64)
    map_fields(out, f"{tag}_cm", side.ChainedKG.feature_map)
    out[f"{tag}_clean_u"], out[f"{tag}_clean_i"], out[f"{tag}_clean_r"] = (clean[c].values.astype(np.int64) for c in ("userId", "itemId", "rating"))

    pos = clean.groupby("userId").cumcount().values
    size = clean.groupby("userId")["itemId"].transform("size").values
    is_test = pos >= size - np.maximum(size // 5, 1)
    out[f"{tag}_is_test"] = is_test.astype(np.int8)
    train = clean[~is_test].reset_index(drop=True)
    data = object.__new__(m.dataset.DataSet)
    data.config = SimpleNamespace(align_side_with_train=True)
    data.side_information = data.align_with_training(train=train, side_information_data=side)
    data.train_dict = data.dataframe_to_dict(train)
    data.users = list(data.train_dict.keys())                                                    # dataset.py:201-217, restated
    data.items = list({k for a in data.train_dict.values() for k in a.keys()})
    data.num_users, data.num_items = len(data.users), len(data.items)
    data.transactions = sum(len(v) for v in data.train_dict.values())
    data.private_users = {p: u for p, u in enumerate(data.users)}
    data.public_users = {v: k for k, v in data.private_users.items()}
    data.private_items = {p: i for p, i in enumerate(data.items)}
    data.public_items = {v: k for k, v in data.private_items.items()}
    data.i_train_dict = {data.public_users[user]: {data.public_items[i]: v for i, v in items.items()}
                         for user, items in data.train_dict.items()}
    data.sp_i_train = data.build_sparse()
    al = data.side_information.ChainedKG
    assert side.ChainedKG.feature_map is not al.feature_map
    out[f"{tag}_al_items"] = np.sort(np.asarray(list(al.object.get_mapped()[1]), np.int64))
    out[f"{tag}_features"] = np.asarray(al.features, np.int64)
    map_fields(out, f"{tag}_am", al.feature_map)
    out[f"{tag}_users"], out[f"{tag}_items"] = np.asarray(data.users, np.int64), np.asarray(data.items, np.int64)
    nF = al.nfeatures
    print(tag, "features: file", len(al.object.feature_names), "coordinated", side.ChainedKG.nfeatures, "aligned", nF, "items",
          len(out[f"{tag}_coord_items"]), "->", len(out[f"{tag}_al_items"]), "of", data.num_items, "transactions", data.transactions)
    if tag == "narrow":
        assert nF % 2 == 1 and nF < 64, nF
        assert side.ChainedKG.nfeatures > nF, "the alignment with the training fold must reduce the map once more"
        assert len(out[f"{tag}_al_items"]) < data.num_items, "some training item must be left without a feature"
    else:
        assert nF > 512, nF

    # ---- the plug-in's constructor: TFIDF, get_profiles, KAHFMModel.initialize ----------------------------------------------------
    def plugin():
        obj = object.__new__(m.plugin.KaHFM)
        obj._data, obj._params, obj.logger = data, SimpleNamespace(**HYPER), log
        obj._num_users, obj._num_items = data.num_users, data.num_items
        obj._seed, obj._epochs = 42, EPOCHS
        obj._batch_size = -1
        m.plugin.KaHFM.__init__(obj, data, None, obj._params)
        return obj
    p = plugin()
    out[f"{tag}_name"] = np.asarray(p.name)
    tf = p._tfidf
    out[f"{tag}_tf_w"] = np.asarray([tf[i][f] for i, fs in al.feature_map.items() for f in fs], np.float64)      # in the order of am_feat
    model = p._model
    out[f"{tag}_P0"], out[f"{tag}_Q0"] = model._user_factors.copy(), model._item_factors.copy()
    last_writer = False
    for u, its in data.train_dict.items():
        seen = {}
        for i in its:
            for f, w in tf.get(i, {}).items():
                last_writer |= f in seen and seen[f] != w
                seen[f] = w
    assert last_writer, "a user with two items that share a feature with different weights"

    # ---- two epochs of KaHFM.train on the reference's own sampler; the fsum twin on the same triplets ------------------------------
    class FsumModel(m.model.KAHFMModel):
        def indexed_predict(self, user, item):
            return self._global_bias + self._item_bias[item] + math.fsum(self._user_factors[user] * self._item_factors[item])
    twin = FsumModel(data, al, tf, p._user_profiles, HYPER["lr"], HYPER["user_regularization"], HYPER["bias_regularization"],
                     HYPER["positive_item_regularization"], HYPER["negative_item_regularization"])
    assert np.array_equal(twin._user_factors, model._user_factors) and np.array_equal(twin._item_factors, model._item_factors)
    sampler = p._sampler
    trip = np.zeros((EPOCHS, 3, data.transactions), np.int32)
    d_reorder, spent = 0.0, 0.0
    for e in range(EPOCHS):
        at = 0
        for batch in sampler.step(data.transactions, p._batch_size):
            n = batch[0].shape[0]
            trip[e, :, at:at + n] = np.stack([b[:, 0] for b in batch])
            at += n
            t0 = time.perf_counter()
            model.train_step(batch)
            spent += time.perf_counter() - t0
            twin.train_step(batch)
        assert at == data.transactions
        state = model.get_model_state()
        for key in ("_user_factors", "_item_factors", "_item_bias"):
            d_reorder = max(d_reorder, float(np.abs(state[key] - twin.get_model_state()[key]).max()))
        tables = {f"{tag}_P_e{e + 1}": state["_user_factors"].copy(), f"{tag}_Q_e{e + 1}": state["_item_factors"].copy(),
                  f"{tag}_b_e{e + 1}": state["_item_bias"].copy()}
        if big:
            path = os.path.join(OUT, f"kahfm_ref_{tag}_e{e + 1}.npz")
            np.savez_compressed(path, **tables)
            print(path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < 1 << 20
        else:
            out.update(tables)
    assert p._batch_size == 10000
    out[f"{tag}_trip"] = trip
    out[f"{tag}_d_reorder"] = np.float64(d_reorder)
    print(tag, "d_reorder", d_reorder, "reference seconds per triplet", spent / (EPOCHS * data.transactions), "at", nF, "features")

    # ---- the reference's lists ---------------------------------------------------------------------------------------------------
    mask = data.sp_i_train.toarray() == 0
    model.prepare_predictions()
    scores = np.where(mask, model._preds, -np.inf)
    top = -np.sort(-scores, axis=1)[:, :K + 1]
    gaps = top[:, :-1] - top[:, 1:]
    assert np.all(np.isfinite(top)) and gaps.min() > 1e-9, gaps.min()             # rank 10 / rank 11 and every pair before them
    idx, val = np.zeros((data.num_users, K), np.int32), np.zeros((data.num_users, K), np.float64)
    for u in data.users:
        recs = model.get_user_predictions(u, mask, K)
        idx[data.public_users[u]] = [data.public_items[x[0]] for x in recs]
        val[data.public_users[u]] = [x[1] for x in recs]
    out[f"{tag}_rec_idx"], out[f"{tag}_rec_val"] = idx, val
    print(tag, "smallest score gap inside the first", K + 1, "ranks", gaps.min())
    if not big:
        model.save_weights(os.path.join(OUT, "kahfm_ref_weights.pkl"))


def main(ref):
    m = load_reference(ref)
    out = dict(k=np.int64(K), threshold=np.int64(THRESHOLD), **{f"hyper_{k}": np.float64(v) for k, v in HYPER.items()})
    _, indices, itd = small_dataset(80, 120, seed=3)
    n_items = int(indices.max()) + 1
    rows = [(u, i, int(r)) for u, d in itd.items() for i, r in d.items()]
    frame = pd.DataFrame(rows, columns=["userId", "itemId", "rating"])
    kg = os.path.join(OUT, "kahfm_kg")
    shutil.rmtree(kg, ignore_errors=True)
    os.makedirs(kg)
    frame.to_csv(os.path.join(kg, "dataset.tsv"), sep="\t", header=False, index=False)
    for tag, spec in CASES.items():
        write_kg_files(os.path.join(kg, tag), *small_kg_features(n_items, **spec))
        run_case(m, tag, frame, os.path.join(kg, tag), out, big=tag == "wide")
    path = os.path.join(OUT, "kahfm_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
