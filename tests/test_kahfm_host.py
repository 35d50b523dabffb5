"""Host half of KaHFM against the reference's own output (tests/golden/kahfm_ref.npz and tests/golden/kahfm_kg/,
scripts/gen_golden_kahfm.py): the ChainedKG loader, its coordination and alignment with the training fold, TF-IDF over the reduced
map and the start tables.  No GPU."""
import numpy as np
import pytest

from elliot_amd.dataset import side_information as si
from elliot_amd.recommender import attribute_profiles as ap
from tests.helpers import kahfm_ref as kr


@pytest.fixture(scope="module")
def cases(golden, tmp_path_factory):
    z = golden("kahfm_ref.npz")
    folder = tmp_path_factory.mktemp("kahfm")
    return {tag: kr.load(z, tag, folder) for tag in kr.CASES}


def write(path, text):
    with open(path, "w") as fh:
        fh.write(text)
    return str(path)


def tiny_kg(tmp_path, features=None, properties="p\n", map_=None):
    """Four items; feature 1 on four of them, 2 on three, 3 on two, 4 on one; 1 and 2 hang on property p, 3 and 4 on q."""
    return {"dataloader": "ChainedKG",
            "map": write(tmp_path / "map.tsv", map_ or "10\t1\t2\t3\t4\n11\t1\t2\t3\n12\t1\t2\n13\t1\n"),
            "features": write(tmp_path / "features.tsv", features or "1\t<p><a>\n2\t<p><b>\n3\t<q><c>\n4\t<q><r><d>\n"),
            "properties": write(tmp_path / "properties.conf", properties)}


def tiny_load(spec, items=(10, 11, 12, 13)):
    return si.ChainedKG.load({1, 2}, set(items), spec, lambda p: p)


# ---- the loader against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", kr.CASES)
def test_coordination_reduces_the_map_as_the_reference_does(cases, tag):
    fx, z = cases[tag], cases[tag].z
    ns = fx.side.ChainedKG
    assert np.array_equal(np.sort(list(ns.object.get_mapped()[1])), z[f"{tag}_coord_items"])
    assert ns.features == z[f"{tag}_coord_features"].tolist() and ns.nfeatures == len(ns.features)
    ref = kr.map_of(z, f"{tag}_cm")
    assert list(ns.feature_map.items()) == list(ref.items())                      # keys and lists in the reference's order
    for col, key in (("userId", "clean_u"), ("itemId", "clean_i"), ("rating", "clean_r")):
        assert np.array_equal(fx.clean[col], z[f"{tag}_{key}"])


@pytest.mark.parametrize("tag", kr.CASES)
def test_alignment_with_the_training_fold_reduces_again(cases, tag):
    fx, z = cases[tag], cases[tag].z
    ns = fx.data.side_information.ChainedKG
    assert np.array_equal(np.sort(list(ns.object.get_mapped()[1])), z[f"{tag}_al_items"])
    assert ns.features == z[f"{tag}_features"].tolist() and ns.nfeatures == z[f"{tag}_features"].shape[0]
    assert ns.private_features == dict(enumerate(ns.features)) and ns.public_features == {f: p for p, f in enumerate(ns.features)}
    assert list(ns.feature_map.items()) == list(kr.map_of(z, f"{tag}_am").items())
    assert set(ns.feature_map) == ns.object.get_mapped()[1]                       # the namespace's map IS the reduced map
    assert fx.data.private_users == dict(enumerate(z[f"{tag}_users"].tolist()))
    assert fx.data.private_items == dict(enumerate(z[f"{tag}_items"].tolist()))
    if tag == "narrow":
        assert ns.nfeatures % 2 == 1 and ns.nfeatures < 64 and ns.nfeatures < fx.side.ChainedKG.nfeatures
        assert len(ns.feature_map) < fx.data.num_items                            # a training item without a feature
    else:
        assert ns.nfeatures > 512


def test_a_fold_owns_its_map(cases):
    fx = cases["narrow"]
    parent = fx.side.ChainedKG
    assert list(parent.feature_map.items()) == list(kr.map_of(fx.z, "narrow_cm").items())      # after the fold was aligned
    fold = parent.object.for_fold()
    assert fold.map_ is not parent.object.map_ and fold.map_ == parent.object.map_
    before = {k: list(v) for k, v in parent.object.map_.items()}
    users, items = fold.get_mapped()
    fold.filter(users, set(list(items)[: len(items) // 2]))
    assert len(fold.map_) < len(before) and parent.object.map_ == before and parent.object.get_mapped()[1] == items


# ---- the loader's rules on a hand-made graph ---------------------------------------------------------------------------------
def test_a_feature_with_exactly_threshold_occurrences_is_dropped(tmp_path):
    ld = tiny_load({**tiny_kg(tmp_path, properties=""), "threshold": 2})
    assert ld.map_ == {10: [1, 2], 11: [1, 2], 12: [1, 2], 13: [1]}               # 3 occurs twice: not MORE than the threshold
    ld = tiny_load({**tiny_kg(tmp_path, properties=""), "threshold": 1})
    assert ld.map_ == {10: [1, 2, 3], 11: [1, 2, 3], 12: [1, 2], 13: [1]}
    assert tiny_load(tiny_kg(tmp_path, properties="")).map_ == {}                  # the default threshold is 10


def test_properties_select_by_the_first_chain_element(tmp_path):
    add = tiny_load({**tiny_kg(tmp_path, properties="# a comment\np\n"), "threshold": 0})
    assert add.map_ == {10: [1, 2], 11: [1, 2], 12: [1, 2], 13: [1]} and add.properties == ["p"]
    sub = tiny_load({**tiny_kg(tmp_path, properties="p\n"), "threshold": 0, "additive": False})
    assert sub.map_ == {10: [3, 4], 11: [3]} and sub.get_mapped()[1] == {10, 11}  # the complement; items without a feature leave
    second = tiny_load({**tiny_kg(tmp_path, properties="r\n"), "threshold": 0})
    assert second.map_ == {}                                                      # r is only a SECOND element (feature 4)
    everything = tiny_load({**tiny_kg(tmp_path, properties="# nothing selected\n"), "threshold": 0})
    assert everything.map_ == {10: [1, 2, 3, 4], 11: [1, 2, 3], 12: [1, 2], 13: [1]}


def test_feature_names_are_cut_as_the_reference_cuts_them(tmp_path):
    path = write(tmp_path / "f.tsv", "1\t<p><a>\n2\t<long><b><c>\n3\t<q><entity>")
    assert si.read_feature_names(path) == {1: ["p", "a"], 2: ["long", "b", "c"], 3: ["q", "entit"]}     # no newline: a real character lost
    single = write(tmp_path / "g.tsv", "7\t<alone>\n8\t<alone>")
    assert si.read_feature_names(single) == {7: ["alone"], 8: ["alon"]}
    # so a last line without a newline changes the selection when its chain has ONE element
    spec = tiny_kg(tmp_path, features="1\t<p>\n2\t<p>", properties="p\n")
    assert tiny_load({**spec, "threshold": 0}).map_ == {10: [1], 11: [1], 12: [1], 13: [1]}


def test_the_map_file_is_read_as_item_attributes_are(tmp_path):
    ld = tiny_load({**tiny_kg(tmp_path, properties="", map_="10\t1\t1\t2\n11\t2\t1\n99\t1\t2\n"), "threshold": 1})
    assert ld.map_ == {10: list({1, 2}), 11: list({2, 1})} and ld.get_mapped()[1] == {10, 11}      # 99 is not rated; 12, 13 have no line


def test_filter_reduces_again(tmp_path):
    ld = tiny_load({**tiny_kg(tmp_path, properties=""), "threshold": 2})
    assert ld.map_[12] == [1, 2]
    ld.filter({1}, {10, 12, 13})                                                  # 2 now occurs twice, 1 three times
    assert ld.map_ == {10: [1], 12: [1], 13: [1]} and ld.get_mapped() == ({1}, {10, 12, 13})
    ld.filter({1}, {10, 12})                                                      # nothing occurs more than twice
    assert ld.map_ == {} and ld.get_mapped() == ({1}, set())
    ns = ld.namespace()
    assert ns.features == [] and ns.nfeatures == 0 and ns.feature_map is ld.map_ and ns.__name__ == "ChainedKG"


@pytest.mark.parametrize("key", ["map", "features", "properties"])
def test_a_missing_key_is_named(tmp_path, key):
    spec = tiny_kg(tmp_path)
    del spec[key]
    with pytest.raises(Exception, match=f"`{key}`"):
        tiny_load(spec)


def test_chained_kg_is_a_registered_loader_and_settles_with_the_frames(tmp_path):
    assert si.LOADERS["ChainedKG"] is si.ChainedKG
    frame = {"userId": np.array([1, 1, 2, 2, 2]), "itemId": np.array([10, 11, 12, 13, 77]), "rating": np.ones(5)}
    clean, side = si.coordinate(frame, [{**tiny_kg(tmp_path, properties=""), "threshold": 2}])
    assert clean["itemId"].tolist() == [10, 11, 12, 13] and side.ChainedKG.nfeatures == 2


# ---- TF-IDF and the start tables ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", kr.CASES)
def test_tfidf_and_start_tables_equal_the_reference_bit_for_bit(cases, tag):
    fx, z = cases[tag], cases[tag].z
    side = fx.data.side_information.ChainedKG
    tf = ap.item_tfidf(side.feature_map)
    w = np.asarray([tf[i][f] for i, fs in side.feature_map.items() for f in fs], np.float64)
    assert kr.same_bits(w, z[f"{tag}_tf_w"])
    P0, Q0 = kr.start_tables(fx.data, side)
    assert kr.same_bits(P0, z[f"{tag}_P0"]) and kr.same_bits(Q0, z[f"{tag}_Q0"])
    assert np.count_nonzero(Q0.any(axis=1)) == len(side.feature_map) and P0.any(axis=1).all()
    F, fw = ap.item_features(fx.data, side, tf)                                   # the operands of ops.kahfm_init
    assert F.shape == Q0.shape and kr.same_bits(fw, Q0[np.repeat(np.arange(F.shape[0]), np.diff(F.indptr)), F.indices])


def test_plugin_needs_its_side_information(cases):
    from types import SimpleNamespace

    from elliot_amd.recommender import KaHFM
    fx = cases["narrow"]
    with pytest.raises(Exception, match="no side information 'ItemAttributes'"):
        KaHFM(data=fx.data, config=fx.cfg, params=SimpleNamespace(meta=SimpleNamespace(verbose=False), loader="ItemAttributes"))
