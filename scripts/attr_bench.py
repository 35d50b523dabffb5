"""Time the attribute kernels: el_profile_build (user profiles) and el_knn_build_f32 (W of float rows), medians of 3.

  ml1m     ML-1M-shaped synthetic ratings (6 040 x 3 706, ~1 M) with a synthetic attribute map: the reference's
           cat_dbpedia_movielens_1m file is not distributed with it, so its statistics are ASSUMED here and can be overridden:
           --features 10000 distinct features, Zipf-distributed, --per-item 20 on average (1 .. 2 x per-item)
             profile_build, modes add (binary) and last (tfidf)
             knn_build_f32 on the resulting tfidf user profiles
             knn_build_f32 beside knn_build (dot) on the SAME binary item x feature matrix
  c2       el_profile_build at BASELINE configs[1] (1 M users x 100 K items, zipf_csr with bench.py's c2 parameters), ~10 features
           per item out of 5 000

Kernel times are the summed hipEvent brackets of the library's own launches (el_timing_enable); call times include the host
side of the wrappers (uploads, the transposition, the copy of the profile matrix back).  One JSON line per measurement on stdout.

Usage:  python scripts/attr_bench.py [--legs ml1m,c2] [--neighbors 50] [--features 10000] [--per-item 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr, zipf_csr_device  # noqa: E402


def item_features(n_items, n_features, per_item, seed):
    """Binary item x feature CSR: 1 .. 2 per_item distinct Zipf-distributed features per item; float64 weights in (0, 1]."""
    rs = np.random.RandomState(seed)
    p = 1.0 / (np.arange(n_features) + 1.0)
    p /= p.sum()
    k = rs.randint(1, 2 * per_item + 1, size=n_items)
    draws = rs.choice(n_features, size=int(k.sum() * 2), p=p)            # with repeats: the first k distinct ones of every item's slice
    rows, pos = [], 0
    for n in k.tolist():
        u = np.unique(draws[pos:pos + 2 * n])
        rows.append(u[rs.permutation(u.shape[0])[:n]])
        pos += 2 * n
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    F = sp.csr_matrix((np.ones(indptr[-1], np.float32), np.concatenate(rows).astype(np.int32), indptr), shape=(n_items, n_features))
    return F, rs.uniform(0.01, 1.0, size=F.nnz)


def kernel_ms(ctx, fn, prefix, reps=3):
    """Median over `reps` runs of the summed times of the kernels whose name starts with one of `prefix`."""
    tot, out = [], None
    for _ in range(reps):
        ctx.timing(True)
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        call = (time.time() - t0) * 1e3
        rep = {n: v for n, v in ctx.timing_report().items() if n.startswith(prefix)}
        ctx.timing(False)
        tot.append((sum(v[1] for v in rep.values()), rep, call))
    tot.sort(key=lambda x: x[0])
    med = tot[len(tot) // 2]
    return {"kernels_ms_median": round(med[0], 3), "kernels_ms_runs": [round(t[0], 3) for t in tot],
            "kernel_breakdown_ms": {n: round(v[1], 3) for n, v in med[1].items()}, "call_ms_runs": [round(t[2], 1) for t in tot]}, out


def profile_leg(ctx, label, ip, ix, F, w):
    visits = int(np.diff(F.indptr)[ix].sum())                            # (user, item, feature) triples: the reference's dict operations
    out = None
    for mode in ("add", "last"):
        fn = lambda: ops.profile_build(ctx, ip, ix, F, w if mode == "last" else None, mode, True)      # noqa: E731
        fn()                                                             # warm-up (first launches)
        t, out = kernel_ms(ctx, fn, "k_profile")
        line = {"leg": label, "kernel": "el_profile_build", "mode": mode, "users": len(ip) - 1, "items": F.shape[0],
                "features": F.shape[1], "ratings": len(ix), "feature_visits": visits, "profile_nnz": int(out.nnz),
                "visits_per_s": round(2 * visits / (t["kernels_ms_median"] / 1e3)), **t, "device": ctx.arch}
        print(json.dumps(line), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m,c2")
    ap.add_argument("--neighbors", type=int, default=50)
    ap.add_argument("--features", type=int, default=10000)
    ap.add_argument("--per-item", type=int, default=20)
    args = ap.parse_args()
    ctx = ops.get_context(0)
    legs = args.legs.split(",")
    N = args.neighbors
    if "ml1m" in legs:
        U, I = 6040, 3706
        ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
        F, w = item_features(I, args.features, args.per_item, seed=4)
        P = profile_leg(ctx, "ml1m", ip, ix, F, w)
        fn = lambda: ops.knn_build_f32(ctx, P, N, "cosine")              # noqa: E731
        fn()
        t, (W, _) = kernel_ms(ctx, fn, "k_knn")
        work = int((np.diff(P.tocsc().indptr).astype(np.int64) ** 2).sum())          # fp64 multiply-adds: sum_t deg(t)^2
        print(json.dumps({"leg": "ml1m", "kernel": "el_knn_build_f32", "rows": "tfidf user profiles", "n": U, "n_other": P.shape[1],
                          "nnz": int(P.nnz), "longest_row": int(np.diff(P.indptr).max()), "neighbors": N, "similarity": "cosine",
                          "multiply_adds": work, "multiply_adds_per_s": round(work / (t["kernels_ms_median"] / 1e3)), **t,
                          "W_nnz": int(W.nnz), "device": ctx.arch}), flush=True)
        A = F.copy()
        A.sort_indices()
        work = int((np.diff(A.tocsc().indptr).astype(np.int64) ** 2).sum())
        for name, fn in (("el_knn_build_f32", lambda: ops.knn_build_f32(ctx, A, N, "dot")),
                         ("el_knn_build", lambda: ops.knn_build(ctx, A, "user", N, "dot"))):
            fn()
            t, (W, _) = kernel_ms(ctx, fn, "k_knn")
            print(json.dumps({"leg": "ml1m", "kernel": name, "rows": "binary item x feature matrix", "n": I, "n_other": A.shape[1],
                              "nnz": int(A.nnz), "neighbors": N, "similarity": "dot", "multiply_adds": work, **t,
                              "W_nnz": int(W.nnz), "device": ctx.arch}), flush=True)
    if "c2" in legs:
        U, I = 1000000, 100000
        ip, ix = zipf_csr_device(U, I, ctx.device, mean_log=3.9, sigma_log=1.0, dmin=5, dmax=2000, seed=1234)
        ip, ix = ip.cpu().numpy(), ix.cpu().numpy()
        F, w = item_features(I, 5000, 10, seed=6)
        profile_leg(ctx, "c2", ip, ix, F, w)


if __name__ == "__main__":
    main()
