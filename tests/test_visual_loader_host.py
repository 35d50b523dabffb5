"""Host: the VisualAttribute loader (elliot_amd/dataset/side_information.py) on a folder that holds files for unrated items, lacks
files for rated ones and, in one test, holds a file of the wrong length."""
import os

import numpy as np
import pytest

from elliot_amd.dataset import side_information as si

D = 6
RATED = [3, 5, 8, 13, 21, 34]                    # item 34 is rated but has no file
IN_FOLDER = [3, 5, 8, 13, 21, 55, 89]            # 55 and 89 have files and no rating


def vector(item):
    return (np.arange(D, dtype=np.float32) + 1) * np.float32(item) / 8


@pytest.fixture()
def folder(tmp_path):
    d = tmp_path / "features"
    d.mkdir()
    for item in IN_FOLDER:
        np.save(d / f"{item}.npy", vector(item))
    (d / "README.txt").write_text("not a feature file")
    return str(d)


def frame():
    users = np.array([1, 1, 1, 2, 2, 3, 3, 3, 4], np.int64)
    items = np.array([3, 5, 34, 8, 13, 21, 3, 34, 5], np.int64)
    return {"userId": users, "itemId": items, "rating": np.ones(len(users), np.float32)}


def spec(folder, **more):
    return {"dataloader": "VisualAttribute", "visual_features": folder, **more}


def test_items_are_the_rated_items_that_have_a_file(folder):
    clean, side = si.coordinate(frame(), [spec(folder)])
    ns = side.VisualAttributes
    assert ns.__name__ == "VisualAttributes" and ns.visual_feature_folder_path == folder and ns.visual_features_shape == D
    users, items = ns.object.get_mapped()
    assert items == {3, 5, 8, 13, 21} and users == {1, 2, 3, 4}
    assert 34 not in clean["itemId"] and set(clean["itemId"].tolist()) == items and len(clean["itemId"]) == 7
    assert set(ns.item_mapping) == set(IN_FOLDER)                                  # the reference's field: every id of the folder ...
    assert sorted(ns.item_mapping.values()) == list(range(len(IN_FOLDER)))         # ... numbered by its position in the folder's set
    assert ns.item_mapping == {item: val for val, item in enumerate(set(IN_FOLDER))}


def test_matrix_rows_follow_the_order_asked_for_and_the_public_file_names(folder):
    _, side = si.coordinate(frame(), [spec(folder)])
    ns = side.VisualAttributes
    order = [13, 3, 21, 5, 8]                                                       # a data set's private-item order
    M = ns.feature_matrix(order)
    assert M.dtype == np.float32 and M.shape == (5, D)
    for row, item in zip(M, order):
        assert np.array_equal(row, vector(item)), f"row of item {item} is not the file {item}.npy"
    assert set(ns.object.store["ids"]) == {3, 5, 8, 13, 21}                        # the unrated items' files were never read
    with pytest.raises(Exception, match="55"):
        ns.feature_matrix([3, 55])


def test_files_are_read_once_by_at_most_16_threads(folder, monkeypatch):
    import threading
    seen, readers, real = [], set(), np.load

    def counting(path, *a, **kw):
        seen.append(os.path.basename(path))
        readers.add(threading.get_ident())
        return real(path, *a, **kw)
    monkeypatch.setattr(np, "load", counting)
    _, side = si.coordinate(frame(), [spec(folder)])
    ns = side.VisualAttributes
    fold = si.align_with_training([1, 2], [3, 5, 8, 13], side).VisualAttributes
    ns.feature_matrix([3, 5]), fold.feature_matrix([8, 13]), fold.feature_matrix([13, 8])
    assert sorted(seen) == sorted(f"{i}.npy" for i in (3, 5, 8, 13, 21))
    assert 1 <= len(readers) <= 16 and si.VisualAttribute.MAX_READERS == 16
    assert fold.object.store is ns.object.store


def test_the_fold_aligned_loader_narrows_with_the_fold(folder):
    _, side = si.coordinate(frame(), [spec(folder)])
    fold = si.align_with_training([1, 2], [3, 5, 8, 13], side).VisualAttributes
    assert fold.object.get_mapped() == ({1, 2}, {3, 5, 8, 13})
    assert side.VisualAttributes.object.get_mapped() == ({1, 2, 3, 4}, {3, 5, 8, 13, 21})        # the loader itself stays as it is
    assert np.array_equal(fold.feature_matrix([13, 3]), np.stack([vector(13), vector(3)]))
    with pytest.raises(Exception, match="21"):
        fold.feature_matrix([21])                                                   # not an item of this fold
    assert fold.visual_features_shape == D and fold.item_mapping is side.VisualAttributes.item_mapping


def test_a_file_of_another_length_is_refused_with_its_name(folder):
    np.save(os.path.join(folder, "8.npy"), np.zeros(D + 1, np.float32))
    with pytest.raises(Exception, match=r"8\.npy"):
        si.coordinate(frame(), [spec(folder)])
    np.save(os.path.join(folder, "8.npy"), vector(8))
    np.save(os.path.join(folder, "89.npy"), np.zeros(D + 1, np.float32))           # an unrated item's file is not read: no complaint
    si.coordinate(frame(), [spec(folder)])


@pytest.mark.parametrize("key", ["visual_pca_features", "visual_feat_map_features", "images_src_folder"])
def test_the_image_models_keys_are_not_supported(folder, key):
    with pytest.raises(Exception, match=f"{key}.*not supported"):
        si.coordinate(frame(), [spec(folder, **{key: folder})])


def test_a_missing_folder_and_an_unknown_loader_are_refused(tmp_path):
    with pytest.raises(Exception, match="visual_features"):
        si.coordinate(frame(), [spec(str(tmp_path / "nowhere"))])
    with pytest.raises(Exception, match="VisualAttribute"):
        si.coordinate(frame(), [{"dataloader": "SentimentInteractionsTextualAttributes"}])
