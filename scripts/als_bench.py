"""iALS step on one MI355X: ms per iteration split into Gram, user half and item half, plus scoring every user at k = 10.

Legs (one JSON line each):
  ml1m     an ML-1M-shaped synthetic set (6 040 x 3 706, ~1 M interactions) at F = 50 and F = 128
  c2       BASELINE configs[1] (1 M users x 100 K items, zipf_csr with bench.py's c2 parameters) at F = 128

Times are hipEvents around each part (median of 3 after one warm-up step).  The fp64 rate counts 2 nnz F^2 per half (the
y y^T sums) plus U F^3 / 3 + I F^3 / 3 (the factorisations) over the two halves' time (the Gram kernels excluded).

Usage:  python scripts/als_bench.py [--legs ml1m,c2] [--k 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr, zipf_csr_device  # noqa: E402

FP64_PEAK_TFLOPS = 78.6      # AMD's published MI355X FP64 vector peak; not measured here


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_leg(ctx, label, indptr, indices, U, I, F, k, reps=3):
    rs = np.random.RandomState(42)
    X = rs.normal(scale=0.01, size=(U, F))
    Y = rs.normal(scale=0.01, size=(I, F))
    st = ops.AlsDeviceState(ctx, X, Y, indptr, indices, 1.0, 2.0, 0.1, gram="fresh")
    del X, Y
    st.step()                                                     # warm-up
    parts = {"gram_y": [], "user_half": [], "gram_x": [], "item_half": []}
    for _ in range(reps):
        parts["gram_y"].append(event_ms(lambda: ops.als_gram(ctx, st.Y, out=st.Gy, holder=st)))
        parts["user_half"].append(event_ms(lambda: ops.als_solve(ctx, st.users, st.Y, st.Gy, st.w_A, st.w_b, st.reg, st.X, holder=st)))
        parts["gram_x"].append(event_ms(lambda: ops.als_gram(ctx, st.X, out=st.Gx, holder=st)))
        parts["item_half"].append(event_ms(lambda: ops.als_solve(ctx, st.items, st.X, st.Gx, st.w_A, st.w_b, st.reg, st.Y,
                                                                   skip_empty=True, holder=st)))
    med = {n: float(np.median(v)) for n, v in parts.items()}
    excl = st.users.csr
    score = sorted(event_ms(lambda: st.recommend(("excl", excl), k, 0, U)) for _ in range(reps))[reps // 2]
    nnz = int(indices.shape[0])
    flops = 2 * (2 * nnz * F * F) + (U + I) * F ** 3 / 3
    halves = med["user_half"] + med["item_half"]
    line = {"leg": label, "U": U, "I": I, "nnz": nnz, "F": F, "ms_per_iteration": round(sum(med.values()), 3),
            **{f"{n}_ms": round(v, 3) for n, v in med.items()}, "all_runs_ms": {n: [round(x, 3) for x in v] for n, v in parts.items()},
            "score_all_users_k10_ms": round(score, 3), "long_rows_items": st.items.n_long, "pieces_items": st.items.n_pieces,
            "fp64_tflops_halves": round(flops / halves / 1e9, 3),
            "fraction_of_published_fp64_peak": round(flops / halves / 1e9 / FP64_PEAK_TFLOPS, 4)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m,c2")
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    ctx = ops.get_context(0)
    if "ml1m" in legs:
        U, I = 6040, 3706
        ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
        for F in (50, 128):
            run_leg(ctx, "ml1m", ip, ix, U, I, F, args.k)
    if "c2" in legs:
        U, I = 1000000, 100000
        ip, ix = zipf_csr_device(U, I, ctx.device, mean_log=3.9, sigma_log=1.0, dmin=5, dmax=2000, seed=1234)
        ip, ix = ip.cpu().numpy(), ix.cpu().numpy()
        run_leg(ctx, "c2", ip, ix, U, I, 128, args.k)


if __name__ == "__main__":
    main()
