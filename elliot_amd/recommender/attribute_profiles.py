"""Host half shared by the attribute-aware baselines (AttributeItemKNN, AttributeUserKNN, VSM): the side information of a data
object as matrices.

Contract of the reference's plug-ins (attribute_item_knn.py, attribute_user_knn.py, vector_space_model.py) and of both
tfidf_utils.py.  The item side (one TF-IDF row per item of the attribute file, I x nF matrices) is host Python in the reference's
own order of operations; the user side -- a dict loop over every (user, item, feature) -- is ops.profile_build.  Two quirks of the
reference are kept, because its results depend on them:
  binary profile of AttributeUserKNN   p[f] += 1 / len(items) once per item that carries f: the repeated addition of one double
                                       (VSM's binary profile is 1 for every feature touched)
  tfidf profile                        TFIDF.get_profiles does NOT sum: its comprehension reads an empty dict, so p[f] is the
                                       weight of f in the LAST item of train_dict[u] that carries f, divided by len(items)
                                       (AttributeUserKNN) or as it is (VSM: the mean of a one-element list)
"""
import math
from collections import Counter

import numpy as np
import scipy.sparse as sp

from .. import ops

PROFILE_TYPES = ("binary", "tfidf")


def side_of(data, loader, who):
    """The namespace of `loader` in data.side_information, or a clear error."""
    side = getattr(getattr(data, "side_information", None), loader, None)
    if side is None:
        raise Exception(f"{who}: the data set carries no side information {loader!r}; configure data_config.side_information "
                        f"with dataloader: {loader} (and its attribute_file)")
    return side


def profile_type(value, who, key):
    if value not in PROFILE_TYPES:
        raise ValueError(f"{who}: {key} {value!r} is not supported; supported: {list(PROFILE_TYPES)}")
    return value


def item_tfidf(feature_map):
    """TFIDF.__init__: {item: {feature: idf / row norm}} over the WHOLE attribute file, Python floats, sums in list order."""
    df = Counter(f for features in feature_map.values() for f in features)
    total = len(feature_map)
    idf = {f: math.log(total / n) for f, n in df.items()}
    out = {}
    for item, features in feature_map.items():
        norm = math.sqrt(sum([idf[f] ** 2 for f in features]))
        out[item] = {f: idf[f] / norm for f in features}
    return out


def item_features(data, side, tfidf=None):
    """(F, w): F scipy CSR [I, nF] float32 over private item and feature ids -- ones, or the TF-IDF weights rounded to float --
    with every row in the order of feature_map[item]; w the same weights as float64 (None without tfidf)."""
    pf = side.public_features
    indptr, cols, w = [0], [], []
    for i in range(data.num_items):
        item = data.private_items[i]
        features = side.feature_map.get(item, [])
        cols.extend(pf[f] for f in features)
        if tfidf is not None:
            row = tfidf.get(item, {})
            w.extend(row.get(f, 0) for f in features)
        indptr.append(len(cols))
    w = np.asarray(w, dtype=np.float64) if tfidf is not None else None
    vals = w.astype(np.float32) if tfidf is not None else np.ones(len(cols), np.float32)
    F = sp.csr_matrix((vals, np.asarray(cols, dtype=np.int32), np.asarray(indptr, dtype=np.int64)),
                      shape=(data.num_items, len(pf)))
    return F, w


def sorted_csr(M):
    """A copy with ascending columns (what the reference's csr_matrix((values, (rows, cols))) stores)."""
    M = M.copy()
    M.sort_indices()
    return M


def train_rows_in_dict_order(data):
    """(indptr, indices) of the train matrix with every row in the order of train_dict[u], private ids."""
    if hasattr(data, "dict_order_csr"):
        return data.dict_order_csr()
    itd = data.i_train_dict                             # a data object of Elliot's own: its dicts are what there is
    lens = [len(itd[u]) for u in range(data.num_users)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return indptr, np.fromiter((i for u in range(data.num_users) for i in itd[u]), dtype=np.int32, count=int(indptr[-1]))


def user_profiles(ctx, data, side, kind, by_len):
    """The user profile matrix [U, nF] float32 CSR (build_feature_sparse_values) on the device kernel.
    kind "binary" with by_len: AttributeUserKNN's repeated addition; without: VSM's ones.  kind "tfidf": last writer wins."""
    indptr, indices = train_rows_in_dict_order(data)
    if kind == "tfidf":
        F, w = item_features(data, side, item_tfidf(side.feature_map))
        return ops.profile_build(ctx, indptr, indices, F, w, "last", by_len)
    F, _ = item_features(data, side)
    if by_len:
        return ops.profile_build(ctx, indptr, indices, F, None, "add", True)
    return ops.profile_build(ctx, indptr, indices, F, np.ones(F.nnz, np.float64), "last", False)


def l2_normalize_rows(M):
    """sklearn's normalize(M) for cosine_similarity, rounded once: every row divided by its fp64 norm; zero rows stay."""
    M = sp.csr_matrix(M, dtype=np.float32)
    d = M.data.astype(np.float64)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    norm = np.sqrt(np.bincount(rows, weights=d * d, minlength=M.shape[0]))
    norm[norm == 0] = 1.0
    return sp.csr_matrix(((d / norm[rows]).astype(np.float32), M.indices, M.indptr), shape=M.shape)
