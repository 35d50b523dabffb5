"""The golden attribute fixture (tests/golden/attr_ref.npz, scripts/gen_golden_attr.py) loaded through this package's own data
plane: the attribute file written back to disk, coordinated with the rating frame, split by the recorded flags, one DataSet."""
import os
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from elliot_amd.dataset.dataset import DataSet, default_config
from elliot_amd.dataset.side_information import coordinate


def write_attribute_file(z, path):
    ip = z["attr_indptr"]
    with open(path, "w") as fh:
        for n, item in enumerate(z["attr_item"].tolist()):
            fh.write("\t".join(str(x) for x in [item] + z["attr_feat"][ip[n]:ip[n + 1]].tolist()) + "\n")


def load(z, folder):
    """SimpleNamespace(z, clean, side, data, cfg, attr_path)."""
    folder = str(folder)
    attr_path = os.path.join(folder, "attributes.tsv")
    write_attribute_file(z, attr_path)
    frame = {"userId": z["rat_u"], "itemId": z["rat_i"], "rating": z["rat_r"]}
    clean, side = coordinate(frame, [{"dataloader": "ItemAttributes", "attribute_file": attr_path}])
    te = z["is_test"].astype(bool)
    cfg = default_config(top_k=10, cutoffs=[10], simple_metrics=["nDCG"], out_dir=os.path.join(folder, "results"))
    for p in (cfg.path_output_rec_result, cfg.path_output_rec_weight):
        os.makedirs(p, exist_ok=True)
    cols = ("userId", "itemId", "rating")
    data = DataSet(cfg, tuple(clean[c][~te] for c in cols), tuple(clean[c][te] for c in cols), side_information=side)
    return SimpleNamespace(z=z, clean=clean, side=side, data=data, cfg=cfg, attr_path=attr_path)


def csr(z, tag):
    return sp.csr_matrix((z[f"{tag}_data"], z[f"{tag}_indices"], z[f"{tag}_indptr"]), shape=tuple(z[f"{tag}_shape"]))


def same_csr(a, b):
    """Bit-equal CSRs (float32 values compared as bits, so a kept zero and its sign count)."""
    a, b = sp.csr_matrix(a), sp.csr_matrix(b)
    return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            and a.data.dtype == b.data.dtype == np.float32 and np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32)))


def w_lists(z, tag):
    """The reference's W columns as [(indices, values)]."""
    wp, wi, wd = z[f"{tag}_w_indptr"], z[f"{tag}_w_indices"], z[f"{tag}_w_data"]
    return [(wi[wp[c]:wp[c + 1]], wd[wp[c]:wp[c + 1]]) for c in range(wp.shape[0] - 1)]


def w_csr(z, tag):
    n = z[f"{tag}_w_indptr"].shape[0] - 1
    W = sp.csc_matrix((z[f"{tag}_w_data"], z[f"{tag}_w_indices"], z[f"{tag}_w_indptr"]), shape=(n, n), dtype=np.float32).tocsr()
    W.sort_indices()
    return W
