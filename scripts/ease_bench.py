"""EASE^R on one MI355X: Gram, LU, inverse, weights and all-user top-10 scoring, per catalogue shape.

Legs (one JSON line each in profiles/ease_bench.jsonl, a table in profiles/ease_bench.md):
  ml1m      ML-1M-shaped synthetic ratings 1..5 (6 040 x 3 706, ~1 M entries, Zipf popularity), l2_norm 1 320
  ml1m_bin  the same pattern, binary
  ml20m     ML-20M-shaped, binary (138 493 x 26 744, ~20 M entries)
  i40k      a 40 000-item catalogue (40 000 users, binary)

Times are hipEvent medians of 3 after one warm-up: gram (el_ease_gram), lu (el_lu_f64 alone, on a copy of G), inverse (el_inv_f64:
the LU plus both triangular solves), weights (el_ease_weights) and scoring (el_csr_dense_scores + el_dense_topk, k = 10, the
train items excluded).  Launch counts come from one extra run under the library's per-launch timing.  fp64 rate: (2/3) n^3 for
the LU plus 2 n^3 for the two triangular solves against n right-hand sides, over the inverse's time, against AMD's published
78.6 TFLOP/s fp64 peak.  Where scoring every user would take minutes, --score-users scores that many users and users/s is
reported from them (the line says so).  --cpu-inv also times the reference's float32 np.linalg.inv on this host's CPU.

Usage:  python scripts/ease_bench.py [--legs ml1m,ml1m_bin,ml20m,i40k] [--score-users 16384] [--cpu-inv]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr  # noqa: E402

FP64_PEAK_TFLOPS = 78.6
LEGS = {"ml1m": (6040, 3706, 4.95, 20, 2000, False, 1320.0), "ml1m_bin": (6040, 3706, 4.95, 20, 2000, True, 1320.0),
        "ml20m": (138493, 26744, 4.6, 20, 5000, True, 1000.0), "i40k": (40000, 40000, 4.3, 20, 5000, True, 1000.0)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(fn, reps):
    return sorted(event_ms(fn) for _ in range(reps))[reps // 2]


def launches(ctx, fn):
    torch.cuda.synchronize()
    ctx.timing_report()
    ctx.timing(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ctx.timing(False)
    return {name: n for name, (n, _ms) in ctx.timing_report().items()}


def kernel_runs_ms(ctx, fn, name, reps):
    """The time of kernel `name` alone (events around its launch, el_timing_enable) in each of `reps` runs of fn."""
    out = []
    torch.cuda.synchronize()
    ctx.timing_report()
    for _ in range(reps):
        ctx.timing(True)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            ctx.timing(False)
        out.append(ctx.timing_report()[name][1])
    return out


def run_leg(ctx, label, reps, score_users, cpu_inv):
    U, I, mean_log, dmin, dmax, binary, l2 = LEGS[label]
    indptr, indices = zipf_csr(U, I, mean_log=mean_log, sigma_log=1.0, dmin=dmin, dmax=dmax, seed=7)
    vals = np.ones(indices.shape[0], np.float32) if binary else \
        np.random.RandomState(3).randint(1, 6, indices.shape[0]).astype(np.float32)
    R = sp.csr_matrix((vals, indices, indptr), shape=(U, I))
    st = ops.EaseDeviceState(ctx, R, l2)
    G = ops.ease_gram(ctx, R, l2)                                                       # warm-up
    gram_ms = [event_ms(lambda: ops.ease_gram(ctx, R, l2, out=G)) for _ in range(reps)]
    t_gram = sorted(gram_ms)[reps // 2]
    gram_kernel_ms = kernel_runs_ms(ctx, lambda: ops.ease_gram(ctx, R, l2, out=G), "k_ease_gram", reps)
    A = torch.empty_like(G)
    ipiv = torch.empty(I, dtype=torch.int32, device=ctx.device)
    ws = torch.empty(int(ctx.lib.el_inv_f64_ws_bytes(I)), dtype=torch.uint8, device=ctx.device)
    lu_ms, inv_ms = [], []
    for r in range(reps + 1):
        A.copy_(G)
        t = event_ms(lambda: ops.lu_f64(ctx, A, ipiv))
        A.copy_(G)
        t2 = event_ms(lambda: ops.inv_f64(ctx, A, ipiv, ws))
        if r:
            lu_ms.append(t)
            inv_ms.append(t2)
    t_lu, t_inv = sorted(lu_ms)[reps // 2], sorted(inv_ms)[reps // 2]
    A.copy_(G)
    n_lu = launches(ctx, lambda: ops.lu_f64(ctx, A, ipiv))
    A.copy_(G)
    n_inv = launches(ctx, lambda: ops.inv_f64(ctx, A, ipiv, ws))
    del G, ws
    B = ops.ease_weights(ctx, A)
    t_w = median(lambda: ops.ease_weights(ctx, A, out=B), reps)
    del A
    torch.cuda.empty_cache()
    st.B = B
    excl = ops.DeviceCSR(indptr, indices, I, ctx.device)
    n_score = U if score_users is None else min(U, score_users)
    st.recommend(("excl", excl), 10, 0, min(n_score, 256))
    t_score = median(lambda: st.recommend(("excl", excl), 10, 0, n_score), reps)
    n = float(I)
    flops = 2.0 / 3.0 * n ** 3 + 2.0 * n ** 3
    line = {"leg": label, "U": U, "I": I, "nnz": int(indices.shape[0]), "binary": binary, "l2_norm": l2,
            "gram_ms": round(t_gram, 3), "lu_ms": round(t_lu, 3), "inverse_ms": round(t_inv, 3),
            "lu_launches": int(sum(n_lu.values())), "inverse_launches": int(sum(n_inv.values())),
            "inverse_launches_by_kernel": n_inv, "lu_tflops_fp64": round(2.0 / 3.0 * n ** 3 / t_lu / 1e9, 2),
            "inverse_tflops_fp64": round(flops / t_inv / 1e9, 2),
            "inverse_pct_of_fp64_peak": round(100.0 * flops / t_inv / 1e9 / FP64_PEAK_TFLOPS, 1),
            "weights_ms": round(t_w, 3), "score_users": n_score, "score_ms": round(t_score, 3),
            "score_users_per_s": round(n_score / t_score * 1e3, 1), "score_all_users": n_score == U,
            "all_runs_ms": {"gram": [round(x, 3) for x in gram_ms], "k_ease_gram": [round(x, 3) for x in gram_kernel_ms],
                            "lu": [round(x, 3) for x in lu_ms], "inverse": [round(x, 3) for x in inv_ms]}}
    if cpu_inv:
        Gh = ease_gram_host(R, l2)
        t0 = time.perf_counter()
        np.linalg.inv(Gh)
        line["cpu_inv_f32_ms_this_host"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(line), flush=True)
    return line


def ease_gram_host(R, l2):
    G = (R.T @ R).toarray().astype(np.float32)
    G[np.diag_indices(G.shape[0])] = np.ediff1d(R.tocsc().indptr) + l2
    return G


def write_md(lines, path):
    rows = ["| leg | U x I | nnz | gram ms | LU ms (launches) | inverse ms (launches) | inverse fp64 TFLOP/s (% of 78.6) | B ms | "
            "scoring ms (users) | users/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for x in lines:
        users = f"{x['score_users']}" + ("" if x["score_all_users"] else " of " + str(x["U"]))
        rows.append(f"| {x['leg']} | {x['U']} x {x['I']} | {x['nnz']} | {x['gram_ms']} | {x['lu_ms']} ({x['lu_launches']}) | "
                    f"{x['inverse_ms']} ({x['inverse_launches']}) | {x['inverse_tflops_fp64']} ({x['inverse_pct_of_fp64_peak']} %) | "
                    f"{x['weights_ms']} | {x['score_ms']} ({users}) | {x['score_users_per_s']} |")
    with open(path, "w") as f:
        f.write("# EASE^R on one MI355X (scripts/ease_bench.py)\n\n" + "\n".join(rows) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m,ml1m_bin,ml20m")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--score-users", type=int, default=None)
    ap.add_argument("--cpu-inv", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ease_bench"))
    a = ap.parse_args()
    ctx = ops.get_context(0)
    lines = []
    for leg in a.legs.split(","):
        lines.append(run_leg(ctx, leg, a.reps, a.score_users if leg in ("ml20m", "i40k") else None, a.cpu_inv))
        torch.cuda.empty_cache()
    with open(a.out + ".jsonl", "a") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")
    write_md(lines, a.out + ".md")


if __name__ == "__main__":
    main()
