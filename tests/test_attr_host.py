"""Host half of the attribute-aware baselines against the reference's own output (tests/golden/attr_ref.npz,
scripts/gen_golden_attr.py): the ItemAttributes loader, its coordination and alignment, TF-IDF, the profile contract, the
plug-ins' names and refusals.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from elliot_amd import ops
from elliot_amd.dataset import side_information as si
from elliot_amd.dataset.dataloader import DataSetLoader
from elliot_amd.dataset.dataset import DataSet
from elliot_amd.recommender import attribute_profiles as ap
from tests.helpers import attr_fixture as fxm
from tests.helpers import attr_ref


@pytest.fixture(scope="module")
def fx(golden, tmp_path_factory):
    return fxm.load(golden("attr_ref.npz"), tmp_path_factory.mktemp("attr"))


def params(**kw):
    return SimpleNamespace(meta=SimpleNamespace(verbose=False), **kw)


# ---- loader ------------------------------------------------------------------------------------------------------------------
def test_coordination_keeps_the_users_and_the_items_of_the_file(fx):
    z, obj = fx.z, fx.side.ItemAttributes.object
    users, items = obj.get_mapped()
    assert np.array_equal(np.sort(list(users)), z["coord_users"]) and np.array_equal(np.sort(list(items)), z["coord_items"])
    assert set(z["rat_i"].tolist()) - items and set(z["attr_item"].tolist()) - set(z["rat_i"].tolist())       # both sides lose items
    for col, key in (("userId", "clean_u"), ("itemId", "clean_i"), ("rating", "clean_r")):
        assert np.array_equal(fx.clean[col], z[key])
    assert fx.side.ItemAttributes.features == z["coord_features"].tolist()


def test_feature_map_is_the_unfiltered_file_in_set_order(fx):
    z, fm = fx.z, fx.data.side_information.ItemAttributes.feature_map
    assert list(fm.keys()) == z["fm_item"].tolist() == z["attr_item"].tolist()
    assert [f for v in fm.values() for f in v] == z["fm_feat"].tolist()
    assert [len(v) for v in fm.values()] == np.diff(z["fm_indptr"]).tolist()
    assert len(z["fm_feat"]) < len(z["attr_feat"])                                    # the repeated features of the file are gone


def test_alignment_with_the_training_fold(fx):
    z, al = fx.z, fx.data.side_information.ItemAttributes
    users, items = al.object.get_mapped()
    assert np.array_equal(np.sort(list(users)), z["al_users"]) and np.array_equal(np.sort(list(items)), z["al_items"])
    assert len(items) < len(z["coord_items"])                                         # the fold does not hold every coordinated item
    assert al.features == z["features"].tolist() and al.nfeatures == len(al.features)
    assert al.features != sorted(al.features)                                         # CPython's set order, not a sorted one
    assert al.private_features == dict(enumerate(al.features))
    assert al.public_features == {f: p for p, f in enumerate(al.features)}
    assert fx.data.users == z["users"].tolist() and fx.data.items == z["items"].tolist()
    # the loader's own namespace is left as it was: another fold aligns from the same start
    assert len(fx.side.ItemAttributes.object.get_mapped()[1]) == len(z["coord_items"])


def test_fixed_point_takes_more_than_one_round(fx, monkeypatch):
    calls = []
    orig = si.ItemAttributes.filter
    monkeypatch.setattr(si.ItemAttributes, "filter", lambda self, u, i: (calls.append((len(u), len(i))), orig(self, u, i))[1])
    frame = {"userId": fx.z["rat_u"], "itemId": fx.z["rat_i"], "rating": fx.z["rat_r"]}
    si.coordinate(frame, [{"dataloader": "ItemAttributes", "attribute_file": fx.attr_path}])
    assert calls == [(len(fx.z["coord_users"]), len(fx.z["coord_items"]))]            # round 1 shrinks and filters, round 2 confirms


def test_align_side_with_train_off_keeps_the_loaders_namespace(fx):
    cfg = SimpleNamespace(**vars(fx.cfg), align_side_with_train=False)
    te = fx.z["is_test"].astype(bool)
    cols = ("userId", "itemId", "rating")
    data = DataSet(cfg, tuple(fx.clean[c][~te] for c in cols), tuple(fx.clean[c][te] for c in cols), side_information=fx.side)
    assert data.side_information is fx.side


def write_frame(path, frame, keep):
    with open(path, "w") as fh:
        for u, i, r in zip(frame["userId"][keep], frame["itemId"][keep], frame["rating"][keep]):
            fh.write(f"{u}\t{i}\t{r}\n")


def test_loader_with_and_without_side_information(fx, tmp_path):
    """strategy: fixed through DataSetLoader: with the attribute file the frames are cleaned after reading; without
    side_information the data set is what it was before this loader existed -- and the rating arrays of the two are the same
    bytes once the input frames are."""
    z = fx.z
    te = z["is_test"].astype(bool)
    raw = {"userId": z["rat_u"], "itemId": z["rat_i"], "rating": z["rat_r"]}
    clean_rows = np.isin(z["rat_i"], z["coord_items"])
    assert np.array_equal(raw["itemId"][clean_rows], z["clean_i"])
    full_te = np.zeros(len(z["rat_u"]), bool)
    full_te[np.flatnonzero(clean_rows)[te]] = True                                    # the dropped rows go to train: they must vanish
    write_frame(tmp_path / "train.tsv", raw, ~full_te)
    write_frame(tmp_path / "test.tsv", raw, full_te)
    write_frame(tmp_path / "train_clean.tsv", fx.clean, ~te)
    write_frame(tmp_path / "test_clean.tsv", fx.clean, te)

    def load(train, test, sides):
        dc = SimpleNamespace(strategy="fixed", train_path=str(tmp_path / train), test_path=str(tmp_path / test))
        if sides:
            dc.side_information = sides
        return DataSetLoader(SimpleNamespace(**vars(fx.cfg), data_config=dc)).generate_dataobjects()[0][0]
    side = [SimpleNamespace(dataloader="ItemAttributes", attribute_file=fx.attr_path)]
    with_side, without = load("train.tsv", "test.tsv", side), load("train_clean.tsv", "test_clean.tsv", None)
    assert vars(without.side_information) == {}
    assert with_side.side_information.ItemAttributes.features == z["features"].tolist()
    for a, b in ((with_side, without), (with_side, fx.data)):
        assert a.users == b.users and a.items == b.items
        for name in ("sp_i_train", "sp_i_train_ratings"):
            A, B = getattr(a, name), getattr(b, name)
            assert A.indptr.tobytes() == B.indptr.tobytes() and A.indices.tobytes() == B.indices.tobytes() \
                and A.data.tobytes() == B.data.tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.split_csr(), b.split_csr()))
    unrated = load("train.tsv", "test.tsv", None)                                     # no side information: nothing is cleaned
    assert unrated.transactions > with_side.transactions and vars(unrated.side_information) == {}


def test_unknown_loader_is_refused(fx):
    frame = {"userId": fx.z["rat_u"], "itemId": fx.z["rat_i"], "rating": fx.z["rat_r"]}
    with pytest.raises(Exception, match="ItemAttributes"):
        si.coordinate(frame, [{"dataloader": "VisualAttribute", "visual_features": "x"}])


# ---- TF-IDF and profiles -----------------------------------------------------------------------------------------------------------
def test_tfidf_weights_equal_the_reference_bit_for_bit(fx):
    fm = fx.data.side_information.ItemAttributes.feature_map
    tf = ap.item_tfidf(fm)
    w = np.asarray([tf[i][f] for i, fs in fm.items() for f in fs], np.float64)
    assert np.array_equal(w.view(np.uint64), fx.z["tf_w"].view(np.uint64))
    assert len(tf) == len(fm) > fx.data.num_items                                     # the document count is the file's, not the fold's


@pytest.fixture(scope="module")
def operands(fx):
    side = fx.data.side_information.ItemAttributes
    ip, ix = ap.train_rows_in_dict_order(fx.data)
    F, _ = ap.item_features(fx.data, side)
    Ft, wt = ap.item_features(fx.data, side, ap.item_tfidf(side.feature_map))
    return SimpleNamespace(ip=ip, ix=ix, F=F, Ft=Ft, wt=wt)


def test_train_rows_follow_train_dict(fx, operands):
    itd = fx.data.i_train_dict
    assert operands.ip.tolist() == np.concatenate([[0], np.cumsum([len(itd[u]) for u in range(fx.data.num_users)])]).tolist()
    assert operands.ix.tolist() == [i for u in range(fx.data.num_users) for i in itd[u]]
    foreign = SimpleNamespace(i_train_dict=itd, num_users=fx.data.num_users)          # a data object of Elliot's own: dicts only
    ip, ix = ap.train_rows_in_dict_order(foreign)
    assert np.array_equal(ip, operands.ip) and np.array_equal(ix, operands.ix)


@pytest.mark.parametrize("tag,kind,by_len", [("auk_binary_A", "binary", True), ("auk_tfidf_A", "tfidf", True),
                                             ("vsm_binary_U", "binary", False), ("vsm_tfidf_U", "tfidf", False)])
def test_profile_contract_equals_the_reference_bit_for_bit(fx, operands, tag, kind, by_len):
    o = operands
    if kind == "tfidf":
        got = attr_ref.profile_matrix(o.ip, o.ix, o.Ft, o.wt, "last", by_len)
    elif by_len:
        got = attr_ref.profile_matrix(o.ip, o.ix, o.F, None, "add", True)
    else:
        got = attr_ref.profile_matrix(o.ip, o.ix, o.F, np.ones(o.F.nnz), "last", False)
    assert fxm.same_csr(got, fxm.csr(fx.z, tag))


def test_last_writer_wins_is_present_in_the_fixture(fx, operands):
    """Last writer wins: some user has two items that share a feature with different weights, so a profile that SUMMED the
    weights differs from the reference's."""
    o = operands
    want = fxm.csr(fx.z, "auk_tfidf_A")
    summed = {}
    for u in range(fx.data.num_users):
        for i in o.ix[o.ip[u]:o.ip[u + 1]]:
            for e in range(o.Ft.indptr[i], o.Ft.indptr[i + 1]):
                summed[(u, int(o.Ft.indices[e]))] = summed.get((u, int(o.Ft.indices[e])), 0.0) + o.wt[e]
    n = np.diff(o.ip)
    differs = sum(np.float32(v / n[u]) != want[u, f] for (u, f), v in summed.items())
    assert differs > 0 and len(summed) == want.nnz


def test_item_matrices_equal_the_reference(fx, operands):
    assert fxm.same_csr(ap.sorted_csr(operands.F), fxm.csr(fx.z, "aik_A"))
    assert fxm.same_csr(ap.sorted_csr(operands.F), fxm.csr(fx.z, "vsm_binary_I"))
    assert fxm.same_csr(ap.sorted_csr(operands.Ft), fxm.csr(fx.z, "vsm_tfidf_I"))


# ---- plug-ins: names and refusals ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """The constructors only store the context; nothing below launches a kernel."""
    monkeypatch.setattr(ops, "get_context", lambda *a, **k: None)


def test_names_equal_the_reference_format(fx, no_device):
    from elliot_amd import recommender as rec
    names = dict(zip(fx.z["name_keys"].tolist(), fx.z["name_values"].tolist()))
    assert len(names) == 6
    for key, want in names.items():
        cls, _, spec = key.partition(":")
        kw = {}
        for part in filter(None, spec.split(",")):
            k, v = part.split("=")
            kw[k] = int(v) if v.isdigit() else {"True": True, "False": False}.get(v, v)
        assert getattr(rec, cls)(data=fx.data, config=fx.cfg, params=params(**kw)).name == want


def test_refusals(fx, no_device):
    from elliot_amd.recommender import AttributeItemKNN, AttributeUserKNN, VSM
    for cls in (AttributeItemKNN, AttributeUserKNN, VSM):
        for sim in ("euclidean", "jaccard", "manhattan"):
            with pytest.raises(ValueError, match="cosine"):
                cls(data=fx.data, config=fx.cfg, params=params(similarity=sim))
    with pytest.raises(ValueError, match="rating matrix"):
        VSM(data=fx.data, config=fx.cfg, params=params(similarity="dot"))
    for kw in ({"user_profile": "counts"}, {"item_profile": "counts"}):
        with pytest.raises(ValueError, match="binary"):
            VSM(data=fx.data, config=fx.cfg, params=params(**kw))
    with pytest.raises(ValueError, match="binary"):
        AttributeUserKNN(data=fx.data, config=fx.cfg, params=params(profile="counts"))
    te = fx.z["is_test"].astype(bool)
    cols = ("userId", "itemId", "rating")
    bare = DataSet(fx.cfg, tuple(fx.clean[c][~te] for c in cols), tuple(fx.clean[c][te] for c in cols))
    for cls in (AttributeItemKNN, AttributeUserKNN, VSM):
        with pytest.raises(Exception, match="side information"):
            cls(data=bare, config=fx.cfg, params=params())
        with pytest.raises(Exception, match="side information"):
            cls(data=fx.data, config=fx.cfg, params=params(loader="VisualAttribute"))


def test_sample_configuration_names_the_three_models():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "config_files", "sample_attribute_knn_amd.yml")) as fh:
        exp = yaml.safe_load(fh)["experiment"]
    assert {"AttributeItemKNN", "AttributeUserKNN", "VSM"} <= {k.split(".")[-1] for k in exp["models"]}
    side = exp["data_config"]["side_information"][0]
    assert side["dataloader"] == "ItemAttributes"
    assert os.path.exists(os.path.join(root, "config_files", side["attribute_file"]))
