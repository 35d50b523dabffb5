"""Generate tests/golden/als_{ials,wrmf}_ref.npz by RUNNING THE REFERENCE'S OWN iALSModel / WRMFModel (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  iALS_model.py and
wrmf_model.py import only numpy / scipy / pickle and are loaded BY FILE PATH.  Every run gets a fresh copy of the data (the
reference's iALSModel writes its confidences into data.sp_i_train) and np.random.seed(42) right before the model is built, as
init_charger does.

One synthetic set (~100 users x 80 items, plus one user and three items without entries).  Every file holds:
  R_indptr / R_indices / shape           the binary train CSR
  <tag>_params                           (factors, alpha, epsilon, reg, scaling: 0 linear, 1 log)   [iALS]  (factors, alpha, reg) [WRMF]
  <tag>_C_data                           the confidences the model holds in C.data (iALS: written into sp_i_train in place)
  <tag>_X_it1 / _Y_it1 / _X_it3 / _Y_it3 X and Y after iterations 1 and 3 (F = 8; the F = 20 variants: iteration 3 only)
  <tag>_rec_idx / _rec_val               get_user_recs(u, allunrated_mask, 10) after iteration 3, padded with (-1, -inf)

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_als.py <reference checkout>
"""
import copy
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

K, SEED, REG = 10, 42, 0.1
IALS = {"lin_a1": (8, 1.0, 1.0, "linear"), "lin_a40": (8, 40.0, 1.0, "linear"), "log_a2_e05": (8, 2.0, 0.5, "log"),
        "lin_a1_f20": (20, 1.0, 1.0, "linear")}
WRMF = {"a1": (8, 1), "a0": (8, 0), "a1_f20": (20, 1)}


def load_by_path(ref, name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_data():
    indptr, indices, _ = small_dataset(100, 80, seed=3)
    U, I = indptr.shape[0] - 1 + 1, int(indices.max()) + 1 + 3          # one empty user, three cold items
    indptr = np.concatenate([indptr, indptr[-1:]]).astype(np.int64)
    B = sp.csr_matrix((np.ones(indices.shape[0], np.float32), indices, indptr), shape=(U, I), dtype=np.float32)
    B.sort_indices()
    ids_u, ids_i = list(range(U)), list(range(I))
    itd = {u: {int(i): 1.0 for i in B.indices[B.indptr[u]:B.indptr[u + 1]]} for u in ids_u}
    return SimpleNamespace(train_dict=itd, sp_i_train=B, num_users=U, num_items=I, users=ids_u, items=ids_i,
                           private_users=dict(enumerate(ids_u)), public_users={u: u for u in ids_u},
                           private_items=dict(enumerate(ids_i)), public_items={i: i for i in ids_i})


def recs(model, U, mask):
    idx = np.full((U, K), -1, np.int32)
    val = np.full((U, K), -np.inf)
    for u in range(U):
        r = model.get_user_recs(u, mask, K)
        idx[u, :len(r)] = [x[0] for x in r]
        val[u, :len(r)] = [x[1] for x in r]
    return idx, val


def dense(m):
    return np.array(m.toarray() if sp.issparse(m) else m, dtype=np.float64)          # a copy: iALS updates X, Y in place


def run(make_model, F, data, out, tag, prepare):
    np.random.seed(SEED)
    model = make_model(copy.deepcopy(data))
    out[f"{tag}_C_data"] = np.asarray(model.C.data, np.float32)
    mask = data.sp_i_train.toarray() == 0
    for it in range(1, 4):
        model.train_step()
        if it in (1, 3) and not (F != 8 and it == 1):
            out[f"{tag}_X_it{it}"], out[f"{tag}_Y_it{it}"] = dense(model.X), dense(model.Y)
    if prepare:
        model.prepare_predictions()
    out[f"{tag}_rec_idx"], out[f"{tag}_rec_val"] = recs(model, data.num_users, mask)


def main(ref):
    if not hasattr(sp.csr_matrix, "A"):          # wrmf_model.py:60 uses `.A`, which scipy 1.14 removed: put the alias back
        sp.csr_matrix.A = property(lambda self: self.toarray())
    data = make_data()
    B = data.sp_i_train
    base = dict(R_indptr=B.indptr.astype(np.int64), R_indices=B.indices.astype(np.int32), shape=np.asarray(B.shape, np.int64),
                k=np.int64(K), seed=np.int64(SEED))
    ials = load_by_path(ref, "ref_ials_model", "elliot/recommender/latent_factor_models/iALS/iALS_model.py")
    out = dict(base)
    for tag, (F, alpha, eps, scaling) in IALS.items():
        out[f"{tag}_params"] = np.asarray([F, alpha, eps, REG, 0 if scaling == "linear" else 1], np.float64)
        run(lambda d: ials.iALSModel(F, d, np.random, alpha, eps, REG, scaling), F, data, out, tag, True)
    path = os.path.join(OUT, "als_ials_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    wrmf = load_by_path(ref, "ref_wrmf_model", "elliot/recommender/latent_factor_models/WRMF/wrmf_model.py")
    out = dict(base)
    for tag, (F, alpha) in WRMF.items():
        out[f"{tag}_params"] = np.asarray([F, alpha, REG], np.float64)
        run(lambda d: wrmf.WRMFModel(F, d, np.random, alpha, REG), F, data, out, tag, False)
    path = os.path.join(OUT, "als_wrmf_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
