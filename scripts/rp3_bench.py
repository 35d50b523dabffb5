"""Time the RP3beta kernels: operands (el_csr_row_l1 + host transposes / powers), el_rp3_rows, el_rp3_cut, and every user's
top-10 (el_knn_score_topk on the built W); hipEvents, medians of 3 after a warm-up.

  ml1m     an ML-1M-shaped synthetic set (6 040 x 3 706, ~1 M integer ratings 1-5: knn_bench.py's generator)
  c2       BASELINE configs[1] (1 M users x 100 K items, zipf_csr with bench.py's c2 parameters)

Two yardsticks are taken in the same process on the same matrix with the same N:
  * el_knn_build (ItemKNN, dot): both builds expand sum_u deg(u)^2 (row, column) pairs, that one with integer LDS atomics in
    any order, this one in scipy's summation order;
  * el_rp3_rows on the single longest row [i, i + 1) against the whole call: a row that dominated the call would mean the
    column slices do not spread it.
One JSON line per leg on stdout.

Usage:  python scripts/rp3_bench.py [--legs ml1m,c2] [--neighbors 50] [--k 10] [--alpha 1.0] [--beta 0.6]
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
    """(median ms, all ms, last result) of `reps` runs bracketed by events on the current stream."""
    out, ms = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(x, 3) for x in ms], out


def host_timed(fn, reps=3):
    """The same on the host clock, for calls that do host work (transposes, powers) before the device's."""
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(x, 1) for x in ms], out


def kernel_breakdown(ctx, fn, prefixes):
    """{kernel: ms} of one run under the library's per-launch events (el_timing_enable)."""
    ctx.timing(True)
    fn()
    torch.cuda.synchronize()
    rep = {n: round(v[1], 3) for n, v in ctx.timing_report().items() if n.startswith(prefixes)}
    ctx.timing(False)
    return rep


def run_leg(ctx, R, N, k, alpha, beta, label):
    U, I = R.shape
    excl = ops.DeviceCSR(R.indptr, R.indices, I, ctx.device)
    Rv = ops.device_values(R.data, ctx.device)
    pairs = int((np.diff(R.indptr).astype(np.int64) ** 2).sum())
    t0 = time.time()
    operands = ops.rp3_operands(ctx, R, alpha, beta)                 # warm-up (first launches) of every stage
    lists = ops.rp3_rows(ctx, *operands, N)
    W, Wv = ops.rp3_cut(ctx, *lists, N, True)
    ops.knn_score_topk(ctx, excl, Rv, W, Wv, 0, min(U, 1024), k, excl=excl)
    torch.cuda.synchronize()
    first_s = time.time() - t0
    operands_ms, operands_all, operands = host_timed(lambda: ops.rp3_operands(ctx, R, alpha, beta))
    rows_ms, rows_all, lists = timed(lambda: ops.rp3_rows(ctx, *operands, N))
    cut_ms, cut_all, (W, Wv) = timed(lambda: ops.rp3_cut(ctx, *lists, N, False))
    cutn_ms, cutn_all, _ = timed(lambda: ops.rp3_cut(ctx, *lists, N, True))
    score_ms, score_all, _ = timed(lambda: ops.knn_score_topk(ctx, excl, Rv, W, Wv, 0, U, k, excl=excl))
    per_item = np.bincount(R.indices, minlength=I)
    longest = int(np.argmax(per_item))
    one_ms, one_all, _ = timed(lambda: ops.rp3_rows(ctx, *operands, N, longest, longest + 1))
    breakdown = kernel_breakdown(ctx, lambda: ops.rp3_cut(ctx, *ops.rp3_rows(ctx, *operands, N), N, True), ("k_rp3", "k_knn"))
    ops.knn_build(ctx, R, "item", N, "dot")                          # the yardstick: warm-up, then its kernels alone
    knn = []
    for _ in range(3):
        rep = kernel_breakdown(ctx, lambda: ops.knn_build(ctx, R, "item", N, "dot"), ("k_knn",))
        knn.append((sum(rep.values()), rep))
    knn.sort(key=lambda x: x[0])
    knn_ms, knn_rep = knn[1]
    line = {"leg": label, "model": "RP3beta", "users": int(U), "items": int(I), "ratings": int(R.nnz), "neighborhood": N, "k": k,
            "alpha": alpha, "beta": beta, "expanded_pairs": pairs,
            "operands_call_ms_incl_host_transposes": round(operands_ms, 1), "operands_ms_runs": operands_all,
            "rp3_rows_ms_median": round(rows_ms, 3), "rp3_rows_ms_runs": rows_all,
            "rp3_cut_ms_median": round(cut_ms, 3), "rp3_cut_ms_runs": cut_all,
            "rp3_cut_normalized_ms_median": round(cutn_ms, 3), "rp3_cut_normalized_ms_runs": cutn_all,
            "score_topk_all_users_ms_median": round(score_ms, 3), "score_ms_runs": score_all,
            "users_per_s": round(U / (score_ms / 1e3)),
            "longest_row": longest, "longest_row_users": int(per_item[longest]),
            "rp3_rows_longest_row_alone_ms_median": round(one_ms, 3), "longest_row_ms_runs": one_all,
            "longest_row_share_of_rows_call": round(one_ms / rows_ms, 4),
            "pairs_per_s_rp3_rows": round(pairs / (rows_ms / 1e3)),
            "kernel_breakdown_ms_rows_plus_normalized_cut": breakdown,
            "knn_build_dot_kernels_ms_median": round(knn_ms, 3), "knn_build_kernel_breakdown_ms": knn_rep,
            "rp3_rows_over_knn_build": round(rows_ms / knn_ms, 3),
            "W_nnz": int(W.nnz), "first_pass_s": round(first_s, 2), "device": ctx.arch}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m,c2")
    ap.add_argument("--neighbors", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=0.6)
    args = ap.parse_args()
    ctx = ops.get_context(0)
    legs = args.legs.split(",")
    if "ml1m" in legs:
        U, I = 6040, 3706
        ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
        rs = np.random.RandomState(3)
        R = sp.csr_matrix((rs.randint(1, 6, size=ix.shape[0]).astype(np.float32), ix, ip), shape=(U, I))
        run_leg(ctx, R, args.neighbors, args.k, args.alpha, args.beta, "ml1m")
    if "c2" in legs:
        U, I = 1000000, 100000
        ip, ix = zipf_csr_device(U, I, ctx.device, mean_log=3.9, sigma_log=1.0, dmin=5, dmax=2000, seed=1234)
        g = torch.Generator(device=ctx.device)
        g.manual_seed(5)
        r = torch.randint(1, 6, (ix.shape[0],), generator=g, device=ctx.device, dtype=torch.int32).to(torch.float32)
        R = sp.csr_matrix((r.cpu().numpy(), ix.cpu().numpy(), ip.cpu().numpy()), shape=(U, I))
        del ip, ix, r
        run_leg(ctx, R, args.neighbors, args.k, args.alpha, args.beta, "c2")


if __name__ == "__main__":
    main()
