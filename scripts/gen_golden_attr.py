"""Generate tests/golden/attr_ref.npz by RUNNING THE REFERENCE'S OWN attribute code (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  Loaded BY FILE PATH
under their own dotted names, and run as they are:
  elliot/dataset/modular_loaders/{abstract_loader, generic/item_attributes, loader_coordinator_mixin}.py
        ItemAttributes, LoaderCoordinator.coordinate_information
  elliot/dataset/dataset.py                DataSet.align_with_training, dataframe_to_dict, build_sparse, build_sparse_ratings (called
                                           on a bare instance: the constructor wants a whole experiment configuration)
  elliot/recommender/base_recommender_model.py     autoset_params, get_params_shortcut (the `name` strings)
  elliot/recommender/knn/attribute_item_knn/*.py, knn/attribute_user_knn/*.py, content_based/VSM/*.py
        the three plug-in constructors (both TFIDF classes, compute_binary_profile, build_feature_sparse*), the three
        Similarity classes (initialize, get_user_recs)
The other `elliot.*` imports of these files (evaluator, splitter, prefilters, negative sampler, logging, RecMixin, write) are
empty stubs, `init_charger` is the identity.  W is captured as scripts/gen_golden_knn.py does, by wrapping `sparse.csc_matrix`.
RESTATED here instead of run, because they sit in the middle of constructors that cannot run without an experiment:
  dataset.py:201-217   users / items / private_ / public_ maps / i_train_dict of a DataSet from its train_dict
The train / test split is this script's own (the last fifth of every user's rows and every row of three rare items, so that the
alignment with the training fold has items to drop), recorded as flags.

Fixture: small_dataset(200, 150, seed=0); an attribute file with 40 Zipf-distributed features, 1-8 per item, a repeated feature
on every tenth line, five rated items missing from it and three lines for items nobody rated.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_attr.py <reference checkout>
"""
import importlib.util
import logging
import os
import sys
import tempfile
import types
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import pandas as pd
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from elliot_amd.synthetic import small_dataset, small_item_attributes  # noqa: E402
from tests.helpers import attr_ref  # noqa: E402

N_NEIGHBORS, K = 20, 10
N_FEATURES = 40
MISSING_ITEMS = (3, 17, 58, 99, 120)          # rated, absent from the attribute file
EXTRA_ITEMS = (5, 9, 20)                      # offsets behind the last rated item: in the file, never rated


def stub(name, **attrs):
    """An empty module under `name` (parents included) with the given attributes."""
    parts = name.split(".")
    for n in range(1, len(parts) + 1):
        key = ".".join(parts[:n])
        if key not in sys.modules:
            m = types.ModuleType(key)
            m.__path__ = []
            sys.modules[key] = m
            if n > 1:
                setattr(sys.modules[".".join(parts[:n - 1])], parts[n - 1], m)
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)
    return sys.modules[name]


def real(ref, name):
    """The reference's own file for the dotted module `name`, executed under that name."""
    stub(name.rsplit(".", 1)[0])
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *name.split(".")) + ".py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)
    return mod


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
    m.item_attributes = real(ref, "elliot.dataset.modular_loaders.generic.item_attributes")
    stub("elliot.dataset.modular_loaders.loaders", ItemAttributes=m.item_attributes.ItemAttributes)
    m.coordinator = real(ref, "elliot.dataset.modular_loaders.loader_coordinator_mixin")
    real(ref, "elliot.dataset.abstract_dataset")
    m.dataset = real(ref, "elliot.dataset.dataset")
    m.base = real(ref, "elliot.recommender.base_recommender_model")
    m.base.init_charger = lambda init: init
    for pkg, files in (("elliot.recommender.knn.attribute_item_knn", ("attribute_item_knn_similarity", "attribute_item_knn")),
                       ("elliot.recommender.knn.attribute_user_knn", ("tfidf_utils", "attribute_user_knn_similarity", "attribute_user_knn")),
                       ("elliot.recommender.content_based.VSM", ("tfidf_utils", "vector_space_model_similarity", "vector_space_model"))):
        for f in files:
            setattr(m, f if f != "tfidf_utils" else pkg.rsplit(".", 1)[1] + "_tfidf", real(ref, f"{pkg}.{f}"))
    return m


class _CaptureSparse:
    """Stands in for `scipy.sparse` inside a loaded similarity module: records csc_matrix's arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(sp, name)

    def csc_matrix(self, arg, *a, **kw):
        data, indices, indptr = arg
        self.calls.append((np.asarray(data, np.float32), np.asarray(indices, np.int32), np.asarray(indptr, np.int64)))
        return sp.csc_matrix(arg, *a, **kw)


def plugin(cls, data, **params):
    """An instance of the reference's plug-in class `cls` whose own constructor ran on `data` (init_charger is the identity, so
    the fields it would have set are given here)."""
    obj = object.__new__(cls)
    obj._data, obj._params, obj.logger = data, SimpleNamespace(**params), logging.getLogger("ref")
    obj._num_users, obj._num_items = data.num_users, data.num_items
    cls.__init__(obj, data, None, obj._params)
    return obj


def csr_fields(out, tag, M):
    M = sp.csr_matrix(M)
    out[f"{tag}_data"], out[f"{tag}_indices"], out[f"{tag}_indptr"] = M.data, M.indices.astype(np.int32), M.indptr.astype(np.int64)
    out[f"{tag}_shape"] = np.asarray(M.shape, np.int64)


def rec_lists(model, data, mask):
    idx = np.full((data.num_users, K), -1, np.int32)
    val = np.full((data.num_users, K), -np.inf, np.float32)
    for u in data.users:
        recs = model.get_user_recs(u, mask, K)
        r = data.public_users[u]
        idx[r, :len(recs)] = [data.public_items[x[0]] for x in recs]
        val[r, :len(recs)] = [x[1] for x in recs]
    return idx, val


def main(ref):
    m = load_reference(ref)
    out = dict(n_neighbors=np.int64(N_NEIGHBORS), k=np.int64(K))

    # ---- the fixture ----------------------------------------------------------------------------------------------------------
    _, indices, itd = small_dataset(200, 150, seed=0)
    n_items = int(indices.max()) + 1
    rows = [(u, i, int(r)) for u, d in itd.items() for i, r in d.items()]
    frame = pd.DataFrame(rows, columns=["userId", "itemId", "rating"])
    out["rat_u"], out["rat_i"], out["rat_r"] = (frame[c].values.astype(np.int64) for c in ("userId", "itemId", "rating"))
    lines = small_item_attributes(n_items, N_FEATURES, MISSING_ITEMS, EXTRA_ITEMS)
    out["attr_item"] = np.asarray([i for i, _ in lines], np.int64)
    out["attr_indptr"] = np.concatenate([[0], np.cumsum([len(f) for _, f in lines])]).astype(np.int64)
    out["attr_feat"] = np.asarray([f for _, fs in lines for f in fs], np.int64)
    tmp = tempfile.mkdtemp()
    attr_path = os.path.join(tmp, "attributes.tsv")
    with open(attr_path, "w") as fh:
        for item, feats in lines:
            fh.write("\t".join(str(x) for x in [item] + feats) + "\n")

    # ---- the reference's loader and coordinator ---------------------------------------------------------------------------------
    side_cfg = SimpleNamespace(dataloader="ItemAttributes", attribute_file=attr_path)
    clean, side = m.coordinator.LoaderCoordinator().coordinate_information(frame, sides=[side_cfg], logger=logging.getLogger("ref"))
    users_c, items_c = side.ItemAttributes.object.get_mapped()
    out["coord_users"], out["coord_items"] = np.sort(np.asarray(list(users_c), np.int64)), np.sort(np.asarray(list(items_c), np.int64))
    out["clean_u"], out["clean_i"], out["clean_r"] = (clean[c].values.astype(np.int64) for c in ("userId", "itemId", "rating"))
    out["coord_features"] = np.asarray(side.ItemAttributes.features, np.int64)
    fmap = side.ItemAttributes.feature_map
    out["fm_item"] = np.asarray(list(fmap.keys()), np.int64)
    out["fm_indptr"] = np.concatenate([[0], np.cumsum([len(v) for v in fmap.values()])]).astype(np.int64)
    out["fm_feat"] = np.asarray([f for v in fmap.values() for f in v], np.int64)

    # ---- this script's split, the reference's alignment and data object ---------------------------------------------------------
    pos = clean.groupby("userId").cumcount().values
    size = clean.groupby("userId")["itemId"].transform("size").values
    is_test = pos >= size - np.maximum(size // 5, 1)
    counts = clean["itemId"].value_counts()
    rare = sorted(counts.index[counts.values == counts.values.min()].tolist())[:3]               # items the training fold never sees
    is_test |= clean["itemId"].isin(rare).values
    out["is_test"] = is_test.astype(np.int8)
    train, test = clean[~is_test].reset_index(drop=True), clean[is_test].reset_index(drop=True)
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
    data.sp_i_train_ratings = data.build_sparse_ratings()
    al = data.side_information.ItemAttributes
    al_users, al_items = al.object.get_mapped()
    assert len(al_items) < len(items_c), "the alignment with the training fold must drop at least one item"
    out["al_users"], out["al_items"] = np.sort(np.asarray(list(al_users), np.int64)), np.sort(np.asarray(list(al_items), np.int64))
    out["features"] = np.asarray(al.features, np.int64)
    out["users"], out["items"] = np.asarray(data.users, np.int64), np.asarray(data.items, np.int64)
    mask = data.sp_i_train.toarray() == 0

    # ---- TF-IDF -------------------------------------------------------------------------------------------------------------
    tf_u = m.attribute_user_knn_tfidf.TFIDF(al.feature_map).tfidf()
    tf_v = m.VSM_tfidf.TFIDF(al.feature_map).tfidf()
    assert tf_u == tf_v
    out["tf_w"] = np.asarray([tf_u[i][f] for i, fs in fmap.items() for f in fs], np.float64)        # in the order of fm_feat

    # ---- AttributeItemKNN ---------------------------------------------------------------------------------------------------------
    names = {}
    cap = _CaptureSparse()
    m.attribute_item_knn_similarity.sparse = cap
    for sim in ("cosine", "dot"):
        p = plugin(m.attribute_item_knn.AttributeItemKNN, data, neighbors=N_NEIGHBORS, similarity=sim)
        csr_fields(out, "aik_A", p._sp_i_features)
        p._model.initialize()
        out[f"aik_{sim}_w_data"], out[f"aik_{sim}_w_indices"], out[f"aik_{sim}_w_indptr"] = cap.calls[-1]
        out[f"aik_{sim}_rec_idx"], out[f"aik_{sim}_rec_val"] = rec_lists(p._model, data, mask)
    names["AttributeItemKNN"] = plugin(m.attribute_item_knn.AttributeItemKNN, data).name
    names["AttributeItemKNN:neighbors=7,similarity=dot,implicit=True"] = \
        plugin(m.attribute_item_knn.AttributeItemKNN, data, neighbors=7, similarity="dot", implicit=True).name

    # ---- AttributeUserKNN ---------------------------------------------------------------------------------------------------------
    cap = _CaptureSparse()
    m.attribute_user_knn_similarity.sparse = cap
    last_writer = False
    for profile in ("binary", "tfidf"):
        for sim in ("cosine", "dot"):
            p = plugin(m.attribute_user_knn.AttributeUserKNN, data, neighbors=N_NEIGHBORS, similarity=sim, profile=profile)
            A = p._sp_i_features
            csr_fields(out, f"auk_{profile}_A", A)
            p._model.initialize()
            tag = f"auk_{profile}_{sim}"
            wd, wi, wp = cap.calls[-1]
            out[f"{tag}_w_data"], out[f"{tag}_w_indices"], out[f"{tag}_w_indptr"] = wd, wi, wp
            out[f"{tag}_rec_idx"], out[f"{tag}_rec_val"] = rec_lists(p._model, data, mask)
            # the measured distance between the reference's float32 chain and the fp64 restatement (DESIGN.md §3.20 quotes it)
            ours = attr_ref.column_lists(A, np.arange(A.shape[0]), N_NEIGHBORS, sim)
            worst = 0.0
            for c, (ox, ov) in enumerate(ours):
                rv = np.sort(wd[wp[c]:wp[c + 1]].astype(np.float64))[::-1]
                assert len(rv) == len(ov), (tag, c)
                if len(rv):
                    worst = max(worst, float(np.max(np.abs(ov.astype(np.float64) - rv) / np.abs(rv))))
            out[f"{tag}_err"] = np.float64(worst)
            out[f"{tag}_L"] = np.int64(np.diff(A.indptr).max())
            print(tag, "max relative distance", worst, "L", int(out[f"{tag}_L"]), "bound", attr_ref.bound(int(out[f"{tag}_L"])))
        if profile == "tfidf":                           # last writer wins: a user with two items that share a feature, other weights
            for u, its in data.train_dict.items():
                seen = {}
                for i in its:
                    for f, w in tf_u.get(i, {}).items():
                        last_writer |= f in seen and seen[f] != w
                        seen[f] = w
    assert last_writer
    names["AttributeUserKNN"] = plugin(m.attribute_user_knn.AttributeUserKNN, data).name
    names["AttributeUserKNN:neighbors=7,profile=tfidf"] = plugin(m.attribute_user_knn.AttributeUserKNN, data, neighbors=7, profile="tfidf").name

    # ---- VSM ----------------------------------------------------------------------------------------------------------------------
    for up in ("binary", "tfidf"):
        for ip in ("binary", "tfidf"):
            p = plugin(m.vector_space_model.VSM, data, similarity="cosine", user_profile=up, item_profile=ip)
            csr_fields(out, f"vsm_{up}_U", p._sp_i_user_features)
            csr_fields(out, f"vsm_{ip}_I", p._sp_i_item_features)
            p._model.initialize()
            tag = f"vsm_{up}_{ip}"
            out[f"{tag}_sim"] = np.array(p._model._similarity_matrix, dtype=np.float32)          # (get_user_recs overwrites its rows)
            out[f"{tag}_rec_idx"], out[f"{tag}_rec_val"] = rec_lists(p._model, data, mask)
    names["VSM"] = plugin(m.vector_space_model.VSM, data).name
    names["VSM:user_profile=binary"] = plugin(m.vector_space_model.VSM, data, user_profile="binary").name
    out["name_keys"], out["name_values"] = np.asarray(list(names.keys())), np.asarray(list(names.values()))

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "attr_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
