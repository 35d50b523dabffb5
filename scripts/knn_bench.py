"""Time the neighbourhood kernels: el_knn_build (W) and el_knn_score_topk (top-10 of every user), hipEvents, median of 3.

  ml1m     ItemKNN and UserKNN on an ML-1M-shaped synthetic set (6 040 x 3 706, ~1 M integer ratings 1-5)
  c2       ItemKNN at BASELINE configs[1] (1 M users x 100 K items, zipf_csr with bench.py's c2 parameters)

Besides the times it reports the bytes the build must read for its row expansion (4 B x sum_t deg(t)^2: every rating of a
row t is read once per entry of t on the target side) as an achieved rate.  One JSON line per measurement on stdout.

Usage:  python scripts/knn_bench.py [--legs ml1m,c2] [--neighbors 50] [--k 10]
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


def timed(fn, reps=3):
    """(median ms, last result) of `reps` runs bracketed by events on the current stream."""
    out, ms = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms, out


def expansion_bytes(R, side):
    """4 B x sum over the other side t of deg(t)^2."""
    deg = np.diff(R.indptr) if side == "item" else np.diff(R.tocsc().indptr)
    return 4 * int((deg.astype(np.int64) ** 2).sum())


def kernel_ms(ctx, fn, reps=3):
    """Median over `reps` runs of the summed k_knn_* kernel times (hipEvents around every launch, el_timing_enable)."""
    tot, out = [], None
    for _ in range(reps):
        ctx.timing(True)
        out = fn()
        torch.cuda.synchronize()
        rep = {n: v for n, v in ctx.timing_report().items() if n.startswith("k_knn")}
        ctx.timing(False)
        tot.append((sum(v[1] for v in rep.values()), rep))
    tot.sort(key=lambda x: x[0])
    med = tot[len(tot) // 2]
    return med[0], [round(t[0], 3) for t in tot], {n: round(v[1], 3) for n, v in med[1].items()}, out


def run_model(ctx, R, side, N, k, label):
    excl = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], ctx.device)
    Rd, Rv = excl, ops.device_values(R.data, ctx.device)
    t0 = time.time()
    ops.knn_build(ctx, R, side, N, "cosine")                     # warm-up (first launches)
    torch.cuda.synchronize()
    first_s = time.time() - t0
    call_ms, _, _ = timed(lambda: ops.knn_build(ctx, R, side, N, "cosine"))
    build_ms, build_all, breakdown, (W, Wv) = kernel_ms(ctx, lambda: ops.knn_build(ctx, R, side, N, "cosine"))
    A, Av, B, Bv = (Rd, Rv, W, Wv) if side == "item" else (W, Wv, Rd, Rv)
    U = R.shape[0]
    score_ms, score_all, _ = timed(lambda: ops.knn_score_topk(ctx, A, Av, B, Bv, 0, U, k, excl=excl))
    kb = expansion_bytes(R, side)
    line = {"leg": label, "model": "ItemKNN" if side == "item" else "UserKNN", "users": int(U), "items": int(R.shape[1]),
            "ratings": int(R.nnz), "neighbors": N, "k": k, "similarity": "cosine",
            "build_kernels_ms_median": round(build_ms, 3), "build_kernels_ms_runs": build_all, "build_kernel_breakdown_ms": breakdown,
            "build_call_ms_incl_host_transposes": round(call_ms, 1),
            "score_topk_all_users_ms_median": round(score_ms, 3), "score_ms_runs": [round(x, 3) for x in score_all],
            "users_per_s": round(U / (score_ms / 1e3)), "expansion_bytes": kb,
            "expansion_rate_GBps": round(kb / (build_ms / 1e3) / 1e9, 1),
            "W_nnz": int(W.nnz), "first_call_s": round(first_s, 2), "device": ctx.arch}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m,c2")
    ap.add_argument("--neighbors", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    ctx = ops.get_context(0)
    legs = args.legs.split(",")
    if "ml1m" in legs:
        U, I = 6040, 3706
        ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
        rs = np.random.RandomState(3)
        R = sp.csr_matrix((rs.randint(1, 6, size=ix.shape[0]).astype(np.float32), ix, ip), shape=(U, I))
        for side in ("item", "user"):
            run_model(ctx, R, side, args.neighbors, args.k, "ml1m")
    if "c2" in legs:
        U, I = 1000000, 100000
        ip, ix = zipf_csr_device(U, I, ctx.device, mean_log=3.9, sigma_log=1.0, dmin=5, dmax=2000, seed=1234)
        g = torch.Generator(device=ctx.device)
        g.manual_seed(5)
        r = torch.randint(1, 6, (ix.shape[0],), generator=g, device=ctx.device, dtype=torch.int32).to(torch.float32)
        R = sp.csr_matrix((r.cpu().numpy(), ix.cpu().numpy(), ip.cpu().numpy()), shape=(U, I))
        del ip, ix, r
        run_model(ctx, R, "item", args.neighbors, args.k, "c2")


if __name__ == "__main__":
    main()
