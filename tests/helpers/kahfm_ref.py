"""The golden KaHFM fixture (tests/golden/kahfm_ref*.npz, tests/golden/kahfm_kg/, scripts/gen_golden_kahfm.py) loaded through this
package's own data plane, and the NumPy restatement of the start tables (KAHFMModel.initialize over TFIDF.get_profiles)."""
import os
from types import SimpleNamespace

import numpy as np

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.dataset.side_information import coordinate
from elliot_amd.recommender import attribute_profiles as ap

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
KG = os.path.join(GOLDEN, "kahfm_kg")
CASES = ("narrow", "wide")


def spec(tag, **kw):
    d = {"dataloader": "ChainedKG", **{k: os.path.join(KG, tag, f) for k, f in (("map", "map.tsv"), ("features", "features.tsv"),
                                                                                 ("properties", "properties.conf"))}}
    return {**d, **kw}


def ratings():
    rows = np.loadtxt(os.path.join(KG, "dataset.tsv"), dtype=np.int64)
    return {"userId": rows[:, 0], "itemId": rows[:, 1], "rating": rows[:, 2]}


def load(z, tag, folder):
    """SimpleNamespace(z, tag, clean, side, data, cfg): the case `tag` coordinated, split by the recorded flags, one DataSet."""
    clean, side = coordinate(ratings(), [spec(tag, threshold=int(z["threshold"]))])
    te = z[f"{tag}_is_test"].astype(bool)
    cfg = default_config(top_k=10, cutoffs=[10], simple_metrics=["nDCG"], out_dir=os.path.join(str(folder), tag))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    cols = ("userId", "itemId", "rating")
    data = DataSet(cfg, tuple(clean[c][~te] for c in cols), tuple(clean[c][te] for c in cols), side_information=side)
    return SimpleNamespace(z=z, tag=tag, clean=clean, side=side, data=data, cfg=cfg)


def map_of(z, tag):
    """{item: [features]} recorded under `tag` (…_item, …_indptr, …_feat), in the reference's order."""
    ip = z[f"{tag}_indptr"]
    return {int(item): z[f"{tag}_feat"][ip[n]:ip[n + 1]].tolist() for n, item in enumerate(z[f"{tag}_item"].tolist())}


def start_tables(data, side):
    """(P0, Q0) float64 as KAHFMModel.initialize fills them: Q0[i, f] = tfidf[i][f]; P0[u, f] = the weight of f in the last item of
    train_dict[u] that carries it, divided by len(train_dict[u]) -- Python floats, one divide per cell."""
    tf = ap.item_tfidf(side.feature_map)
    pf = side.public_features
    indptr, indices = ap.train_rows_in_dict_order(data)
    P0, Q0 = np.zeros((data.num_users, len(pf))), np.zeros((data.num_items, len(pf)))
    for i in range(data.num_items):
        for f, v in tf.get(data.private_items[i], {}).items():
            Q0[i, pf[f]] = v
    for u in range(data.num_users):
        row = indices[indptr[u]:indptr[u + 1]]
        last = {}
        for i in row.tolist():
            last.update(tf.get(data.private_items[i], {}))
        for f, v in last.items():
            P0[u, pf[f]] = v / len(row)
    return P0, Q0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
