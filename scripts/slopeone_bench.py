"""SlopeOne on one MI355X: the deviation build beside el_ease_gram on the same matrix, the scoring table and all-user scoring.

Legs (one JSON line each in profiles/slopeone_bench.jsonl, a table in profiles/slopeone_bench.md):
  ml1m   ML-1M-shaped synthetic ratings 1..5 (6 040 x 3 706, ~1 M entries, Zipf popularity)
  c2     BASELINE configs[1]'s shape (1 M users x 100 K items): 20 I^2 bytes = 200 GB of freq, dev and T; only where memory allows

Times are hipEvent medians of 3 after one warm-up:
  build    el_slope_build (freq, dev and T from its epilogue); beside it el_ease_gram on the same matrix -- the same expansion
           with one counter per cell and one fp64 store per cell instead of two counters and an int32 + two fp64 stores
  table    el_slope_table (T again, from freq and dev: what a restored checkpoint pays)
  scores   el_slope_scores over --score-users users (default: all); reported as bytes of T read, nnz(rows scored) * I * 8,
           per second, against the 8.6 TB/s that MI355X_MICROARCH.md measures for random rows gathered out of the Infinity Cache
  recommend  scores + el_dense_topk_f64 (k = 10, the train items excluded) + padding: users/s
Recorded, not gated.

Usage:  python scripts/slopeone_bench.py [--legs ml1m] [--score-users N]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr  # noqa: E402

INFINITY_CACHE_GATHER_TBS = 8.6
LEGS = {"ml1m": (6040, 3706, 4.95, 20, 2000), "c2": (1_000_000, 100_000, 3.0, 5, 2000)}


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


def kernel_ms(ctx, fn, name, reps):
    """Median time of kernel `name` alone (events around its launch) over `reps` runs of fn."""
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
    return sorted(out)[reps // 2]


def run_leg(ctx, label, reps, score_users):
    U, I, mean_log, dmin, dmax = LEGS[label]
    indptr, indices = zipf_csr(U, I, mean_log=mean_log, sigma_log=1.0, dmin=dmin, dmax=dmax, seed=7)
    rs = np.random.RandomState(3)
    vals = rs.randint(1, 6, indices.shape[0]).astype(np.float64)
    R = sp.csr_matrix((vals, indices, indptr), shape=(U, I))
    order = np.concatenate([a + rs.permutation(b - a) for a, b in zip(indptr[:-1], indptr[1:])])     # a shuffled dict order
    st = ops.SlopeDeviceState(ctx, R, (indptr, indices[order]))
    st.build()                                                                                        # warm-up
    t_build = kernel_ms(ctx, lambda: ops.slope_build(ctx, R, freq=st.freq, dev=st.dev), "k_slope_build", reps)
    G = ops.ease_gram(ctx, R, 0.0)
    t_gram = kernel_ms(ctx, lambda: ops.ease_gram(ctx, R, 0.0, out=G), "k_ease_gram", reps)
    del G
    T2 = ops.slope_table(ctx, st.freq, st.dev)
    t_table = median(lambda: ops.slope_table(ctx, st.freq, st.dev, out=T2), reps)
    assert torch.equal(T2.view(torch.int64), st.T.view(torch.int64))
    del T2
    torch.cuda.empty_cache()
    n = U if score_users is None else min(U, score_users)
    P = torch.empty((min(n, st.block_rows), I), dtype=torch.float64, device=ctx.device)

    def scores():
        for s in range(0, n, st.block_rows):
            ops.slope_scores(ctx, st.rows, st.user_mean, st.T, s, min(s + st.block_rows, n), out=P)
    scores()
    t_scores = median(scores, reps)
    excl = ops.DeviceCSR(indptr, indices, I, ctx.device)
    st.recommend(("excl", excl), 10, 0, min(n, 256))
    t_rec = median(lambda: st.recommend(("excl", excl), 10, 0, n), reps)
    t_bytes = float(indptr[n]) * I * 8.0
    line = {"leg": label, "U": U, "I": I, "nnz": int(indices.shape[0]), "build_ms": round(t_build, 3),
            "ease_gram_ms": round(t_gram, 3), "build_over_gram": round(t_build / t_gram, 2), "table_ms": round(t_table, 3),
            "score_users": n, "scores_ms": round(t_scores, 3), "t_bytes_read": t_bytes,
            "t_read_tb_per_s": round(t_bytes / t_scores / 1e9, 3),
            "pct_of_infinity_cache_gather": round(100.0 * t_bytes / t_scores / 1e9 / INFINITY_CACHE_GATHER_TBS, 1),
            "recommend_ms": round(t_rec, 3), "recommend_users_per_s": round(n / t_rec * 1e3, 1)}
    print(json.dumps(line), flush=True)
    return line


def write_md(lines, path):
    rows = ["| leg | U x I | nnz | build ms | el_ease_gram ms | build / gram | table ms | scores ms (users) | T read TB/s "
            f"(% of {INFINITY_CACHE_GATHER_TBS}) | recommend ms | users/s |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for x in lines:
        rows.append(f"| {x['leg']} | {x['U']} x {x['I']} | {x['nnz']} | {x['build_ms']} | {x['ease_gram_ms']} | {x['build_over_gram']} | "
                    f"{x['table_ms']} | {x['scores_ms']} ({x['score_users']}) | {x['t_read_tb_per_s']} "
                    f"({x['pct_of_infinity_cache_gather']} %) | {x['recommend_ms']} | {x['recommend_users_per_s']} |")
    with open(path, "w") as f:
        f.write("# SlopeOne on one MI355X (scripts/slopeone_bench.py)\n\n" + "\n".join(rows) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--score-users", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "slopeone_bench"))
    a = ap.parse_args()
    ctx = ops.get_context(0)
    lines = [run_leg(ctx, leg, a.reps, a.score_users) for leg in a.legs.split(",")]
    with open(a.out + ".jsonl", "a") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")
    write_md(lines, a.out + ".md")


if __name__ == "__main__":
    main()
