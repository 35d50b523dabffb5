"""Generate tests/golden/puresvd_ref.npz by RUNNING THE REFERENCE'S OWN PureSVDModel.train_step (build machine only).

TEST INFRASTRUCTURE.  Needs sklearn and the reference checkout (argument or $ELLIOT_REF); nothing at test time reads either.
elliot/recommender/latent_factor_models/PureSVD/pure_svd_model.py is loaded BY FILE PATH (the package's __init__ imports
TensorFlow); it imports numpy, scipy and sklearn only.

Fixtures: clustered-Bernoulli binary matrices, gen(U, I, density, seed) below (own code), CASES = (U, I, factors, density, fixture
seed, model seed): both orientations (U < I and U > I), both n_iter values, and one shape twice with two model seeds.  Per case
<tag> the file holds
  <tag>_shape / _indptr / _indices, _factors, _seed    the binary CSR (all values 1), the hyper-parameter and the model seed
  <tag>_sigma32, _sigma64                               the singular values of the float32 run (what the reference computes) and
                                                        of the same code on the float64 copy of the matrix
  <tag>_D                                               max |P_ref32 - P_ref64|, P = user_vec item_vec^T
  <tag>_t64                                             the float64 run's orthonormal table T = Q U^ on the rows of M (M = A, or A^T
                                                        when U < I): user_vec, or item_vec / sigma when U < I.  The other table is
                                                        M^T T by construction of the method (diag(s) Vt = U^T M), so
                                                        tests/helpers/psvd_ref.py::ref64_tables rebuilds both; stored as float64 for
                                                        the small cases and as its float32 rounding above FULL64 entries (the file
                                                        has to stay below 1 MiB)
  <tag>_rebuild_err                                     max |P_ref64 - rebuilt P_ref64| as measured here (tests add it to their error)
  <tag>_user32 / _item32                                the reference's float32 tables (small cases only)
  <tag>_top64                                           every user's masked top-10 under P_ref64 (int16, score desc, index asc)
  <tag>_top32_rows / _top32_lists                       the users whose list under P_ref32 differs from it, and their lists
  <tag>_row_err                                         every user's largest |P_ref32 - P_ref64|
Asserted here, because the tests rely on it: rank >= factors + 10; no empty row or column; the users whose two lists differ
are at most 2 % of the case; the reference's user_vec is sklearn's U and its item_vec is (diag(s) Vt)^T bit for bit.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_puresvd.py <reference checkout> [--time] [--time-only]
  --time: also time sklearn's randomized_svd at the ML-1M shape (scripts/puresvd_bench.py's ml1m pattern, factors 50) on this CPU.
"""
import importlib.util
import os
import sys
import time
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from tests.helpers import psvd_ref  # noqa: E402

REL = "elliot/recommender/latent_factor_models/PureSVD/pure_svd_model.py"
# (U, I, factors, density, fixture seed, model seed)
CASES = [(300, 200, 10, 0.08, 1, 42),
         (200, 320, 10, 0.06, 2, 42),
         (400, 250, 32, 0.05, 3, 42),
         (150, 120, 16, 0.10, 4, 42),
         (1000, 600, 50, 0.03, 5, 42),
         (600, 900, 100, 0.03, 6, 42),
         (150, 120, 16, 0.10, 4, 7)]
FULL64 = 12000            # cases with at most this many table entries keep t64 in float64 and the reference's float32 tables
K = 10
ML1M = dict(n_users=6040, n_items=3706, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)


def tag_of(U, I, f, seed):
    return f"u{U}_i{I}_f{f}_s{seed}"


def gen(U, I, dens, seed, c=12):
    r = np.random.RandomState(seed)
    gu, gi = r.randint(0, c, U), r.randint(0, c, I)
    pop = (1.0 / np.arange(1, I + 1) ** 0.5)[r.permutation(I)]
    p = (r.rand(c, c) ** 3)[gu][:, gi] * pop[None, :]
    p = np.clip(p / p.mean() * dens + 0.3 * dens, 0, 1)
    A = (r.rand(U, I) < p).astype("float32")
    for u in np.flatnonzero(A.sum(1) == 0):
        A[u, r.randint(I)] = 1.0
    for i in np.flatnonzero(A.sum(0) == 0):
        A[r.randint(U), i] = 1.0
    return A


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_pure_svd_model", os.path.join(ref, REL))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_tables(mod, A, factors, seed):
    U, I = A.shape
    ids_u, ids_i = {u: u for u in range(U)}, {i: i for i in range(I)}
    data = SimpleNamespace(sp_i_train=A, private_users=ids_u, public_users=ids_u, private_items=ids_i, public_items=ids_i,
                           train_dict={}, num_users=U, num_items=I)
    m = mod.PureSVDModel(factors, data, seed)
    m.train_step()
    return np.asarray(m.user_vec), np.asarray(m.item_vec)


def write_golden(mod):
    from sklearn.utils.extmath import randomized_svd
    os.makedirs(OUT, exist_ok=True)
    out, tags = {}, []
    for U, I, f, dens, fseed, seed in CASES:
        tag = tag_of(U, I, f, seed)
        dense = gen(U, I, dens, fseed)
        assert dense.sum(1).min() > 0 and dense.sum(0).min() > 0, tag
        rank = np.linalg.matrix_rank(dense.astype(np.float64))
        assert rank >= f + 10, (tag, rank)
        A32 = sp.csr_matrix(dense, dtype=np.float32)
        A32.sort_indices()
        A64 = sp.csr_matrix(A32, dtype=np.float64)
        u32, i32 = reference_tables(mod, A32, f, seed)
        u64, i64 = reference_tables(mod, A64, f, seed)
        assert u32.dtype == np.float32 and i32.dtype == np.float32 and u64.dtype == np.float64, (u32.dtype, i32.dtype, u64.dtype)
        sig = {}
        for A, key, uu, ii in ((A32, "32", u32, i32), (A64, "64", u64, i64)):
            Us, s, Vt = randomized_svd(A, n_components=f, random_state=seed)
            assert np.array_equal(Us, uu) and np.array_equal((sp.diags(s) * Vt).T, ii), (tag, key)
            sig[key] = np.asarray(s, np.float64)
        P32 = psvd_ref.scores(u32, i32)
        P64 = psvd_ref.scores(u64, i64)
        diff = np.abs(P32 - P64)
        D = float(diff.max())
        top32, _ = psvd_ref.topk(P32, A32.indptr, A32.indices, K)
        top64, _ = psvd_ref.topk(P64, A32.indptr, A32.indices, K)
        differ = int((top32 != top64).any(1).sum())
        assert differ <= 0.02 * U, (tag, differ)
        weak = psvd_ref.fragile(P32, diff.max(1), A32.indptr, A32.indices, K)
        full = (U + I) * f <= FULL64
        t64 = i64 / sig["64"][None, :] if U < I else u64
        stored = t64 if full else t64.astype(np.float32)
        probe = {f"{tag}_t64": stored, f"{tag}_sigma64": sig["64"]}
        rebuild_err = float(np.abs(psvd_ref.scores(*psvd_ref.ref64_tables(probe, tag, A64)) - P64).max())
        assert rebuild_err <= 0.05 * D, (tag, rebuild_err, D)
        out[f"{tag}_shape"] = np.asarray([U, I], np.int64)
        out[f"{tag}_indptr"], out[f"{tag}_indices"] = A32.indptr.astype(np.int32), A32.indices.astype(np.int16)
        out[f"{tag}_factors"], out[f"{tag}_seed"] = np.int64(f), np.int64(seed)
        out[f"{tag}_sigma32"], out[f"{tag}_sigma64"] = sig["32"], sig["64"]
        out[f"{tag}_D"], out[f"{tag}_rebuild_err"] = np.float64(D), np.float64(rebuild_err)
        out[f"{tag}_t64"] = stored
        if full:
            out[f"{tag}_user32"], out[f"{tag}_item32"] = u32, i32
        rows = np.flatnonzero((top32 != top64).any(1))
        out[f"{tag}_top64"] = top64.astype(np.int16)
        out[f"{tag}_top32_rows"], out[f"{tag}_top32_lists"] = rows.astype(np.int32), top32[rows].astype(np.int16)
        out[f"{tag}_row_err"] = diff.max(1)
        tags.append(tag)
        rel = np.abs(sig["32"] - sig["64"]).max() / sig["64"].max()
        print(f"{tag}: nnz {A32.nnz}, rank {rank}, plan {psvd_ref.plan(U, I, f)}, D {D:.3g}, sigma f32 vs f64 rel {rel:.2g}, lists that "
              f"differ {differ}, fragile {int(weak.sum())} of {U}, t64 as {'float64' if full else 'float32'}, rebuild error "
              f"{rebuild_err / D:.3g} D", flush=True)
    out["cases"] = np.asarray(tags)
    path = os.path.join(OUT, "puresvd_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def time_reference():
    from sklearn.utils.extmath import randomized_svd
    from elliot_amd.synthetic import zipf_csr
    indptr, indices = zipf_csr(**ML1M)
    A = sp.csr_matrix((np.ones(indices.shape[0], np.float32), indices, indptr), shape=(ML1M["n_users"], ML1M["n_items"]))
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        randomized_svd(A, n_components=50, random_state=42)
        times.append(time.perf_counter() - t0)
    print(f"sklearn randomized_svd at {A.shape[0]} x {A.shape[1]}, nnz {A.nnz}, factors 50 on this CPU ({os.cpu_count()} logical "
          f"CPUs): median {np.median(times):.3f} s of {[round(t, 3) for t in times]}", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--time-only" not in sys.argv:
        write_golden(load_reference(args[0] if args else os.environ["ELLIOT_REF"]))
    if "--time" in sys.argv or "--time-only" in sys.argv:
        time_reference()
