"""Generate tests/golden/slim_ref.npz by RUNNING sklearn's ElasticNet AND THE REFERENCE'S OWN SlimModel.train (build machine only).

TEST INFRASTRUCTURE.  Needs sklearn and the reference checkout (argument or $ELLIOT_REF); nothing at test time reads either.
elliot/recommender/latent_factor_models/Slim/slim_model.py is loaded BY FILE PATH (the package's __init__ imports TensorFlow);
it imports numpy, scipy and sklearn only.

One synthetic set, small_dataset(300, 120, seed=0, mean_log=3.2, sigma_log=0.6, dmin=8, dmax=100) (the RP3beta fixture), ratings
("rat") and its binarisation ("bin"); seed 42.  Cases (matrix, alpha, l1_ratio, neighborhood, exclusion) = CASES:
  column cases     one ElasticNet (the reference's arguments, slim_model.py:30-39) per target on the CSC with column j zeroed
  reference cases  the reference's SlimModel.train(); the weights before its cut come from ElasticNet on the matrix with user
                   row j zeroed, and the generator asserts that their cut IS the reference's W_sparse
The file holds
  R_data / R_indices / R_indptr / shape, seed   the input CSR (ratings; the binary matrix is R with data = 1)
  cases, tag_params [n, 3]                      the tags in order; (alpha, l1_ratio, neighborhood)
  <tag>_c32_rows / _cols / _data                sklearn's float32 weights before the cut, sparse: row = target j, col = item i
  <tag>_c64_rows / _cols / _data                the same from float64 X and y (the yardstick of the tolerance rule)
  <tag>_n_iter, _n_iter64                       sklearn's sweeps per target
  <tag>_w_data / _w_indices / _w_indptr         W after the cut, float32 CSR [I, I]
  <tag>_same32, _same64                         per target: tests/helpers/slim_ref.py stops at sklearn's sweep
Asserted here, because the tests rely on it: no cut falls inside a tie; wherever the restatement stops at sklearn's sweep its
weights equal sklearn's bit for bit (float32 and float64); on PINNED cases it does so on every column; the cut binds where
the tests say it does.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_slim.py <reference checkout> [--time [N]] [--time-only]
  --time: also time the reference's per-item fit (its ElasticNet, its zeroing) on N (default 8) evenly spread items at the
  ML-1M shape (zipf_csr(6040, 3706), ratings 1..5) on this CPU and extrapolate to the whole loop.
"""
import importlib.util
import os
import sys
import time
import warnings
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from elliot_amd.synthetic import small_dataset, zipf_csr  # noqa: E402
from tests.helpers import slim_ref  # noqa: E402

REL = "elliot/recommender/latent_factor_models/Slim/slim_model.py"
FIXTURE = dict(n_users=300, n_items=120, seed=0, mean_log=3.2, sigma_log=0.6, dmin=8, dmax=100)
SEED = 42
# (tag, binary, alpha, l1_ratio, neighborhood, exclusion)
CASES = [("rat_a0.01_l0.1_n10", False, 0.01, 0.1, 10, "column"),
         ("bin_a0.05_l0.5_n20", True, 0.05, 0.5, 20, "column"),
         ("rat_a1_l0.01_n10", False, 1.0, 0.01, 10, "column"),
         ("rat_a0.001_l0.001_n10", False, 0.001, 0.001, 10, "column"),
         ("ref_a0.001_l0.001_n10", False, 0.001, 0.001, 10, "reference"),
         ("ref_a0.01_l0.1_n10", False, 0.01, 0.1, 10, "reference")]
PINNED = {"rat_a0.01_l0.1_n10", "bin_a0.05_l0.5_n20", "rat_a1_l0.01_n10", "ref_a0.001_l0.001_n10", "ref_a0.01_l0.1_n10"}
ML1M = dict(n_users=6040, n_items=3706, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)   # scripts/slim_bench.py's ml1m


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_slim_model", os.path.join(ref, REL))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_model(mod, R, alpha, l1_ratio, N):
    U, I = R.shape
    return mod.SlimModel(SimpleNamespace(sp_i_train_ratings=R), U, I, l1_ratio, alpha, 1, N, SEED)


def fixture_matrix():
    indptr, indices, itd = small_dataset(**FIXTURE)
    rows = [u for u, d in itd.items() for _ in d]
    cols = [i for d in itd.values() for i in d]
    vals = [r for d in itd.values() for r in d.values()]
    R = sp.csr_matrix((np.asarray(vals, np.float32), (rows, cols)), shape=(len(itd), int(indices.max()) + 1), dtype=np.float32)
    R.sum_duplicates()
    R.sort_indices()
    return R


def sklearn_fit(md, X, j, exclusion):
    """(weights, sweeps) of the reference's estimator on the regressor matrix of target j."""
    md.fit(slim_ref.masked(X, j, exclusion), X[:, j].toarray())
    return np.asarray(md.coef_).ravel().copy(), int(np.ravel(md.n_iter_)[0])


def sparse_triple(out, key, coef):
    rows, cols = np.nonzero(coef)
    out[f"{key}_rows"], out[f"{key}_cols"], out[f"{key}_data"] = rows.astype(np.int32), cols.astype(np.int32), coef[rows, cols]


def main(ref, timing=None, generate=True):
    warnings.filterwarnings("ignore")                            # ConvergenceWarning: columns that run out of sweeps are data here
    mod = load_reference(ref)
    if generate:
        write_golden(mod)
    if timing:
        time_reference(mod, timing)


def write_golden(mod):
    os.makedirs(OUT, exist_ok=True)
    R0 = fixture_matrix()
    U, I = R0.shape
    assert np.diff(R0.tocsc().indptr).min() > 0, "the fixture has an empty column"
    out = dict(R_data=R0.data, R_indices=R0.indices.astype(np.int32), R_indptr=R0.indptr.astype(np.int64),
               shape=np.asarray(R0.shape, np.int64), seed=np.int64(SEED))
    tags, tag_params = [], []
    for tag, binary, alpha, l1_ratio, N, exclusion in CASES:
        R = R0.copy()
        if binary:
            R.data[:] = 1.0
        md = reference_model(mod, R, alpha, l1_ratio, N).md      # the reference's own ElasticNet object
        same = {}
        coefs = {}
        for dtype, key in ((np.float32, "32"), (np.float64, "64")):
            X = sp.csc_matrix(R, dtype=dtype)
            X.sort_indices()
            coef = np.zeros((I, I), dtype)
            n_iter = np.zeros(I, np.int32)
            for j in range(I):
                coef[j], n_iter[j] = sklearn_fit(md, X, j, exclusion)
                assert coef[j].dtype == dtype
            rc, rn = slim_ref.fit(R, alpha, l1_ratio, SEED, exclusion, dtype)
            same[key] = rn == n_iter
            for j in np.flatnonzero(same[key]):
                assert np.array_equal(rc[j], coef[j]), (tag, key, j)
            coefs[key] = coef
            sparse_triple(out, f"{tag}_c{key}", coef)
            out[f"{tag}_n_iter" + ("" if key == "32" else "64")] = n_iter
            out[f"{tag}_same{key}"] = same[key]
        if tag in PINNED:
            assert same["32"].all() and same["64"].all(), (tag, int(same["32"].sum()), int(same["64"].sum()))
        W, ties = slim_ref.w_from_coef(coefs["32"], N)
        assert ties == 0, (tag, ties)
        if exclusion == "reference":
            me = reference_model(mod, R.copy(), alpha, l1_ratio, N)
            me.train(False)
            Wr = sp.csr_matrix(me._w_sparse)
            Wr.sort_indices()
            assert np.array_equal(W.indptr, Wr.indptr) and np.array_equal(W.indices, Wr.indices) and \
                np.array_equal(slim_ref.bits(W.data), slim_ref.bits(Wr.data)), tag
            diag = coefs["32"][np.arange(I), np.arange(I)]
            print(f"  reference fit: W[j, j] is the column's largest weight on {int((coefs['32'].argmax(1) == np.arange(I)).sum())} of {I}"
                  f" columns, mean {diag.mean():.4f}; largest other weight {np.where(np.eye(I, dtype=bool), 0, coefs['32']).max():.4g}")
        out[f"{tag}_w_data"], out[f"{tag}_w_indices"], out[f"{tag}_w_indptr"] = W.data, W.indices.astype(np.int32), \
            W.indptr.astype(np.int64)
        nnz = (coefs["32"] != 0).sum(1)
        binds = int((nnz - 1 > N).sum())
        if binary:
            assert 0 < binds < I, (tag, binds)
        tags.append(tag)
        tag_params.append([alpha, l1_ratio, N])
        tol, d_ref = slim_ref.tolerance(coefs["32"], coefs["64"])
        print(f"{tag}: nnz(W) = {W.nnz}, cut binds on {binds} of {I} columns, same sweep f32 {int(same['32'].sum())} f64 "
              f"{int(same['64'].sum())}, sweeps mean {out[f'{tag}_n_iter'].mean():.1f} max {out[f'{tag}_n_iter'].max()}, "
              f"D_ref {d_ref:.3g}, max|W64| {np.abs(coefs['64']).max():.3g}, tied cuts 0")
    out["cases"] = np.asarray(tags)
    out["tag_params"] = np.asarray(tag_params, np.float64)
    path = os.path.join(OUT, "slim_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def time_reference(mod, n_items):
    indptr, indices = zipf_csr(**ML1M)
    ratings = np.random.RandomState(3).randint(1, 6, size=indices.shape[0]).astype(np.float32)
    R = sp.csr_matrix((ratings, indices, indptr), shape=(ML1M["n_users"], ML1M["n_items"]))
    for alpha, l1_ratio in ((0.001, 0.001), (0.01, 0.1)):
        md = reference_model(mod, R, alpha, l1_ratio, 10).md
        items = np.linspace(0, R.shape[1] - 1, n_items).astype(int)
        t0 = time.perf_counter()
        sweeps = []
        for j in items:                                          # slim_model.py:59-69 for one item
            y = R[:, j].toarray()
            s, e = R.indptr[j], R.indptr[j + 1]
            keep = R.data[s:e].copy()
            R.data[s:e] = 0.0
            md.fit(R, y)
            R.data[s:e] = keep
            sweeps.append(int(np.ravel(md.n_iter_)[0]))
        dt = time.perf_counter() - t0
        print(f"reference fit at {R.shape[0]} x {R.shape[1]}, nnz {R.nnz}, alpha {alpha} l1_ratio {l1_ratio}: {dt / n_items:.2f} s per "
              f"item over {n_items} items (sweeps mean {np.mean(sweeps):.1f}), extrapolated {dt / n_items * R.shape[1]:.0f} s for "
              f"train()'s {R.shape[1]} items", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    timing = None
    if "--time" in sys.argv:
        k = sys.argv.index("--time")
        timing = int(sys.argv[k + 1]) if k + 1 < len(sys.argv) and sys.argv[k + 1].isdigit() else 8
        args = [a for a in args if not (a.isdigit() and sys.argv.index(a) == k + 1)]
    main(args[0] if args else os.environ["ELLIOT_REF"], timing=timing, generate="--time-only" not in sys.argv)
