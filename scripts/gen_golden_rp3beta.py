"""Generate tests/golden/rp3beta_ref.npz by RUNNING THE REFERENCE'S OWN RP3beta.train (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.
elliot/recommender/graph_based/RP3beta/rp3beta.py is loaded BY FILE PATH with the two `elliot.recommender.*` modules it
imports stubbed (a base class without behaviour and an identity `init_charger`).  Its W_sparse is captured by wrapping
`sparse.csc_matrix` in the loaded module's namespace: the (data, indices, indptr) it is called with are recorded, the loops that
build them are not restated.  Pui, Piu and degree are read from the trained object.

One synthetic set, small_dataset(300, 120, seed=0, mean_log=3.2, sigma_log=0.6, dmin=8, dmax=100), ratings ("rat") and its
binarisation ("bin"); cases (neighborhood, alpha, beta, normalize_similarity) = CASES on both, plus (-1, 1, 0.6, False) on the
ratings.  The file holds
  R_data / R_indices / R_indptr / shape      the input CSR (ratings; the binary matrix is R with data = 1)
  piu_indices / piu_indptr                   structure of Piu (the same for every case)
  cases                                      the tags, in order; tag_params [n, 4]
  <ops>_pui_data, _piu_data                  the reference's finished operands (after the alpha power), <ops> = the tag's
                                             first two fields (matrix, alpha): cases that share them share the arrays
  <tag>_degree                               the reference's degree (fp64)
  <tag>_w_data / _w_indices / _w_indptr      the reference's W_sparse columns (CSC arguments)
  <tag>_rec_idx / _rec_val                   get_user_predictions(u, all-unrated mask, 10) for every user
The comparison with the reference's W means something only where no cut falls inside a tie (its argsort breaks ties as its
introsort happens to): the generator asserts 0 tied cuts for every case with the restatement in tests/helpers/rp3_ref.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_rp3beta.py <reference checkout> [--time]
  --time: also time the reference's train() at the ML-1M shape (zipf_csr(6040, 3706), neighborhood 50) on this CPU.
"""
import importlib.util
import os
import sys
import time
import types
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from elliot_amd.synthetic import small_dataset, zipf_csr  # noqa: E402
from tests.helpers import rp3_ref  # noqa: E402

K = 10
REL = "elliot/recommender/graph_based/RP3beta/rp3beta.py"
FIXTURE = dict(n_users=300, n_items=120, seed=0, mean_log=3.2, sigma_log=0.6, dmin=8, dmax=100)
CASES = [(10, 1., 0.6, False), (10, 0.8, 0.3, True), (20, 1., 0., False)]
FULL = (-1, 1., 0.6, False)
ML1M = dict(n_users=6040, n_items=3706, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)   # scripts/rp3_bench.py's ml1m


def load_reference(ref):
    """The reference's module with its two package imports stubbed; returns (module, capture)."""
    for name in ("elliot", "elliot.recommender", "elliot.recommender.base_recommender_model",
                 "elliot.recommender.recommender_utils_mixin"):
        sys.modules.setdefault(name, types.ModuleType(name))
    base = sys.modules["elliot.recommender.base_recommender_model"]
    base.BaseRecommenderModel = type("BaseRecommenderModel", (), {})
    base.init_charger = lambda f: f
    sys.modules["elliot.recommender.recommender_utils_mixin"].RecMixin = type("RecMixin", (), {})
    spec = importlib.util.spec_from_file_location("ref_rp3beta", os.path.join(ref, REL))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cap = _CaptureSparse()
    mod.sparse = cap
    mod.print = lambda *a, **k: None
    return mod, cap


class _CaptureSparse:
    """Stands in for `scipy.sparse` inside the loaded module: records csc_matrix's (data, indices, indptr) arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(sp, name)

    def csc_matrix(self, arg, *a, **kw):
        if isinstance(arg, tuple) and len(arg) == 3:
            data, indices, indptr = arg
            self.calls.append((np.asarray(data, np.float32), np.asarray(indices, np.int32), np.asarray(indptr, np.int64)))
        return sp.csc_matrix(arg, *a, **kw)


def train_reference(mod, R, N, alpha, beta, norm):
    """A reference RP3beta object after its own train() on R."""
    U, I = R.shape
    ids_u, ids_i = list(range(U)), list(range(I))
    data = SimpleNamespace(sp_i_train_ratings=R, items=ids_i, users=ids_u, num_items=I,
                           public_users={u: u for u in ids_u}, private_items=dict(enumerate(ids_i)))
    me = object.__new__(mod.RP3beta)
    me._restore, me._data = False, data
    me._neighborhood, me._alpha, me._beta, me._normalize_similarity = (I if N == -1 else N), alpha, beta, norm
    me.evaluate = lambda: None
    me.train()
    return me


def fixture_matrix():
    indptr, indices, itd = small_dataset(**FIXTURE)
    rows = [u for u, d in itd.items() for _ in d]
    cols = [i for d in itd.values() for i in d]
    vals = [r for d in itd.values() for r in d.values()]
    R = sp.csr_matrix((np.asarray(vals, np.float32), (rows, cols)), shape=(len(itd), int(indices.max()) + 1), dtype=np.float32)
    R.sum_duplicates()
    R.sort_indices()
    return R


def tag_of(binary, case):
    N, alpha, beta, norm = case
    return f"{'bin' if binary else 'rat'}_n{N if N != -1 else 'all'}_a{alpha:g}_b{beta:g}_{'norm' if norm else 'raw'}"


def ops_of(tag):
    """Key of a case's operand arrays: its matrix and alpha."""
    f = tag.split("_")
    return f"{f[0]}_{f[2]}"


def main(ref, timing=False):
    os.makedirs(OUT, exist_ok=True)
    mod, cap = load_reference(ref)
    R0 = fixture_matrix()
    U, I = R0.shape
    mask = np.asarray(R0.toarray() == 0)
    out = dict(R_data=R0.data, R_indices=R0.indices.astype(np.int32), R_indptr=R0.indptr.astype(np.int64),
               shape=np.asarray(R0.shape, np.int64), k=np.int64(K))
    tags, tag_params = [], []
    todo = [(b, c) for b in (False, True) for c in CASES] + [(False, FULL)]
    for binary, case in todo:
        N, alpha, beta, norm = case
        R = R0.copy()
        if binary:
            R.data[:] = 1.0
        me = train_reference(mod, R.copy(), N, alpha, beta, norm)
        wd, wi, wp = cap.calls[-1]
        tag = tag_of(binary, case)
        tags.append(tag)
        tag_params.append([N, alpha, beta, float(norm)])
        Piu = me.Piu.tocsr()
        assert Piu.has_sorted_indices and me.Pui.dtype == np.float32 and Piu.dtype == np.float32 and me.degree.dtype == np.float64
        assert np.array_equal(me.Pui.indices, R.indices) and np.array_equal(me.Pui.indptr, R.indptr)
        if "piu_indices" in out:
            assert np.array_equal(out["piu_indices"], Piu.indices) and np.array_equal(out["piu_indptr"], Piu.indptr)
        out["piu_indices"], out["piu_indptr"] = Piu.indices.astype(np.int32), Piu.indptr.astype(np.int64)
        ops = ops_of(tag)
        if f"{ops}_pui_data" in out:
            assert np.array_equal(out[f"{ops}_pui_data"], me.Pui.data) and np.array_equal(out[f"{ops}_piu_data"], Piu.data)
        out[f"{ops}_pui_data"], out[f"{ops}_piu_data"], out[f"{tag}_degree"] = me.Pui.data, Piu.data, me.degree
        out[f"{tag}_w_data"], out[f"{tag}_w_indices"], out[f"{tag}_w_indptr"] = wd, wi, wp
        # the condition of the comparison: no cut inside a tie, and then the restatement IS the reference's W
        Pui = sp.csr_matrix((me.Pui.data, R.indices, R.indptr), shape=R.shape)
        W, row_ties, col_ties = rp3_ref.build_w(Piu, Pui, me.degree, N, norm)
        assert row_ties == 0 and col_ties == 0, (tag, row_ties, col_ties)
        Wr = sp.csc_matrix((wd, wi, wp), shape=(I, I), dtype=np.float32).tocsr()
        Wr.sort_indices()
        assert np.array_equal(W.indptr, Wr.indptr) and np.array_equal(W.indices, Wr.indices) and \
            np.array_equal(W.data.view(np.uint32), Wr.data.view(np.uint32)), tag
        idx = np.full((U, K), -1, np.int32)
        val = np.full((U, K), -np.inf, np.float32)
        for u in range(U):
            recs = me.get_user_predictions(u, mask, K)
            idx[u, :len(recs)] = [r[0] for r in recs]
            val[u, :len(recs)] = [r[1] for r in recs]
        out[f"{tag}_rec_idx"], out[f"{tag}_rec_val"] = idx, val
        print(tag, "nnz(W) =", wd.shape[0], "tied cuts: 0")
    out["cases"] = np.asarray(tags)
    out["tag_params"] = np.asarray(tag_params, np.float64)
    path = os.path.join(OUT, "rp3beta_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    if timing:
        indptr, indices = zipf_csr(**ML1M)
        ratings = np.random.RandomState(3).randint(1, 6, size=indices.shape[0]).astype(np.float32)
        R = sp.csr_matrix((ratings, indices, indptr), shape=(ML1M["n_users"], ML1M["n_items"]))
        t0 = time.perf_counter()
        train_reference(mod, R, 50, 1., 0.6, False)
        print(f"reference train() at {R.shape[0]} x {R.shape[1]}, nnz {R.nnz}, neighborhood 50: {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else os.environ["ELLIOT_REF"], timing="--time" in sys.argv)
