"""Generate tests/golden/ease_ref.npz by RUNNING THE REFERENCE'S OWN EASER.train (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  ease_r.py is loaded
BY FILE PATH with stub modules for elliot.recommender.base_recommender_model / recommender_utils_mixin (the package's own import
chain needs TensorFlow).  The model is built with object.__new__; train() runs with _data.sp_i_train_ratings, _l2_norm and a
no-op evaluate().  Before anything is written, the restatement R.dot(B) (scipy) must equal the reference's _preds bit for bit.

Cases (240 users x 84 items each; <tag>_R_indptr / _R_indices / _R_data / _shape, <tag>_l2):
  rat_l5      ratings 1..5, l2_norm 5: G is indefinite (pivoting is required)                       + <tag>_B (reference float32 B)
  rat_l1320   ratings 1..5, l2_norm 1320                                                              + <tag>_B
  bin_l50     the binary matrix, l2_norm 50                                                           + <tag>_B
  cold_item   ratings, one item without entries, l2_norm 10
  empty_user  ratings, one user without entries, l2_norm 10
<tag>_rec_idx / _rec_val: get_user_predictions(u, all-unrated mask, 10), padded with (-1, -inf); _rec_val only where no B is
stored (with B, the scores are R.dot(B) exactly).

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_ease.py <reference checkout>
"""
import importlib.util
import logging
import os
import sys
import types
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "ease_ref.npz")
K = 10
CASES = {"rat_l5": (False, 5.0, None), "rat_l1320": (False, 1320.0, None), "bin_l50": (True, 50.0, None),
         "cold_item": (False, 10.0, "item"), "empty_user": (False, 10.0, "user")}
WITH_B = ("rat_l5", "rat_l1320", "bin_l50")


def load_reference(ref):
    base = types.ModuleType("elliot.recommender.base_recommender_model")
    base.BaseRecommenderModel = type("StubBase", (), {})
    base.init_charger = lambda f: f
    mixin = types.ModuleType("elliot.recommender.recommender_utils_mixin")
    mixin.RecMixin = type("StubMixin", (), {})
    for name in ("elliot", "elliot.recommender"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules[base.__name__] = base
    sys.modules[mixin.__name__] = mixin
    spec = importlib.util.spec_from_file_location("ref_ease_r", os.path.join(ref, "elliot/recommender/autoencoders/EASE_R/ease_r.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_matrix(seed, binary, hole):
    rs = np.random.RandomState(seed)
    U, I = 240, 84
    pop = 1.0 / np.arange(1, I + 1) ** 0.6                      # Zipf-like popularity
    p = np.minimum(0.35, 0.12 * pop / pop.mean())
    M = (rs.rand(U, I) < p[rs.permutation(I)][None, :]) * rs.randint(1, 6, (U, I))
    M[np.arange(U), rs.randint(0, I, U)] = rs.randint(1, 6, U)     # every user rates something
    if hole == "item":
        M[:, 7] = 0
    if hole == "user":
        M[11, :] = 0
    if binary:
        M = (M > 0).astype(int)
    R = sp.csr_matrix(M.astype(np.float32))
    R.sort_indices()
    return R


def main(ref):
    mod = load_reference(ref)
    out = {"k": np.int64(K)}
    for seed, (tag, (binary, l2, hole)) in enumerate(CASES.items()):
        R = make_matrix(100 + seed, binary, hole)
        U, I = R.shape
        m = object.__new__(mod.EASER)
        m._restore = False
        m._l2_norm = l2
        m.logger = logging.getLogger("gen_golden_ease")
        m.evaluate = lambda *a, **kw: None
        m._data = SimpleNamespace(sp_i_train_ratings=R, public_users={u: u for u in range(U)},
                                  private_items={i: i for i in range(I)})
        m.train()
        B, preds = m._similarity_matrix, np.array(m._preds)
        assert B.dtype == np.float32 and preds.dtype == np.float32
        mine = R.dot(B)
        assert mine.dtype == np.float32 and np.array_equal(mine.view(np.int32), preds.view(np.int32)), tag
        mask = R.toarray() == 0
        idx = np.full((U, K), -1, np.int32)
        val = np.full((U, K), -np.inf, np.float32)
        for u in range(U):
            r = m.get_user_predictions(u, mask, K)
            idx[u, :len(r)] = [x[0] for x in r]
            val[u, :len(r)] = [x[1] for x in r]
        out.update({f"{tag}_R_indptr": R.indptr.astype(np.int64), f"{tag}_R_indices": R.indices.astype(np.int32),
                    f"{tag}_R_data": R.data.astype(np.float32), f"{tag}_shape": np.asarray(R.shape, np.int64),
                    f"{tag}_l2": np.float64(l2), f"{tag}_rec_idx": idx})
        if tag in WITH_B:
            out[f"{tag}_B"] = B
        else:
            out[f"{tag}_rec_val"] = val
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
