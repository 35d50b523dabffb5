"""Generate tests/golden/knn_{item,user}_ref.npz by RUNNING THE REFERENCE'S OWN Similarity classes (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  The modules
item_knn_similarity.py / user_knn_similarity.py import only numpy / scipy / sklearn and are loaded BY FILE PATH.  Their W is
captured by wrapping `sparse.csc_matrix` in the loaded module's namespace: the (data, indices, indptr) it is called with are
recorded, the loop that builds them is not restated.

For {cosine, dot} x {implicit False, True} on one synthetic set (integer ratings 1-5) every file holds:
  R_data / R_indices / R_indptr / shape       the input CSR (ratings; the binary matrix is R with data = 1)
  <sim>_<bin>_w_data / _w_indices / _w_indptr  the reference's W columns (CSC, column c = c's neighbours)
  <sim>_<bin>_rec_idx / _rec_val               get_user_recs(u, allunrated_mask, k) for every user, padded with (-1, -inf)

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_knn.py <reference checkout>
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from elliot_amd.synthetic import small_dataset  # noqa: E402

N_NEIGHBORS, K = 20, 10
FILES = {"item": ("knn_item_ref.npz", "elliot/recommender/knn/item_knn/item_knn_similarity.py"),
         "user": ("knn_user_ref.npz", "elliot/recommender/knn/user_knn/user_knn_similarity.py")}


def load_by_path(ref, name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _CaptureSparse:
    """Stands in for `scipy.sparse` inside the loaded module: records csc_matrix's arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(sp, name)

    def csc_matrix(self, arg, *a, **kw):
        data, indices, indptr = arg
        self.calls.append((np.asarray(data, np.float32), np.asarray(indices, np.int32), np.asarray(indptr, np.int64)))
        return sp.csc_matrix(arg, *a, **kw)


def fake_data(itd, U, I):
    rows = [u for u, d in itd.items() for _ in d]
    cols = [i for d in itd.values() for i in d]
    vals = [r for d in itd.values() for r in d.values()]
    R = sp.csr_matrix((np.asarray(vals, np.float32), (rows, cols)), shape=(U, I), dtype=np.float32)
    R.sum_duplicates()
    R.sort_indices()
    B = R.copy()
    B.data[:] = 1.0
    ids_u, ids_i = list(range(U)), list(range(I))
    return SimpleNamespace(train_dict=itd, sp_i_train=B, sp_i_train_ratings=R, users=ids_u, items=ids_i,
                           private_users=dict(enumerate(ids_u)), public_users={u: u for u in ids_u},
                           private_items=dict(enumerate(ids_i)), public_items={i: i for i in ids_i})


def main(ref):
    os.makedirs(OUT, exist_ok=True)
    indptr, indices, itd = small_dataset(200, 150, seed=0)
    U, I = len(itd), int(indices.max()) + 1
    data = fake_data(itd, U, I)
    R = data.sp_i_train_ratings
    mask = data.sp_i_train.toarray() == 0
    for side, (fname, rel) in FILES.items():
        mod = load_by_path(ref, f"ref_{side}_knn_similarity", rel)
        cap = _CaptureSparse()
        mod.sparse = cap
        out = dict(R_data=R.data, R_indices=R.indices.astype(np.int32), R_indptr=R.indptr.astype(np.int64),
                   shape=np.asarray(R.shape, np.int64), n_neighbors=np.int64(N_NEIGHBORS), k=np.int64(K))
        for sim in ("cosine", "dot"):
            for implicit in (False, True):
                tag = f"{sim}_{'bin' if implicit else 'rat'}"
                model = mod.Similarity(data=data, num_neighbors=N_NEIGHBORS, similarity=sim, implicit=implicit)
                model.initialize()
                wd, wi, wp = cap.calls[-1]
                out[f"{tag}_w_data"], out[f"{tag}_w_indices"], out[f"{tag}_w_indptr"] = wd, wi, wp
                idx = np.full((U, K), -1, np.int32)
                val = np.full((U, K), -np.inf, np.float32)
                for u in range(U):
                    recs = model.get_user_recs(u, mask, K)
                    idx[u, :len(recs)] = [r[0] for r in recs]
                    val[u, :len(recs)] = [r[1] for r in recs]
                out[f"{tag}_rec_idx"], out[f"{tag}_rec_val"] = idx, val
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
