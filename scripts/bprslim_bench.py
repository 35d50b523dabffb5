"""BPRSlim on one MI355X at the ML-1M shape: the level schedule, one epoch of el_bprslim_apply_levels, el_bprslim_table, all users'
scores and top-10 -- beside KaHFM's epoch at 1 024 factors and el_slope_scores on the same matrix, the two nearest existing kernels.

  ratings    ML-1M-shaped synthetic ratings (6 040 x 3 706, 944 497 entries; zipf_csr with the parameters of scripts/kahfm_bench.py)
  triplets   one epoch = as many Philox triplets as ratings (el_bpr_sample, seed 42)
  schedule   el_bprslim_levels_host (rows i and j only) beside el_bprsgd_levels_host (user, i and j) on the same triplets: levels,
             their mean and largest size, the host time
  epoch      el_bprslim_apply_levels from the call to the synchronize behind it, WITHOUT event brackets, median of 3 after a warm-up
             epoch (the triplets are on the device in level order); the summed hipEvent brackets of the same launches in a
             further epoch; the bytes of S the kernel moves (per seen item two cells read twice and written once: 48 bytes)
  table      el_bprslim_table, hipEvent median of 3
  scores     el_bprslim_scores for all users (blocks of <= 256 MiB), hipEvent median of 3, as bytes of St read per second
             (nnz * I * 8) against the 8.6 TB/s MI355X_MICROARCH.md measures for rows gathered out of the Infinity Cache
  recommend  scores + el_dense_topk_f64 (k = 10, train items excluded) + padding
  kahfm      one epoch of el_bprsgd_apply_levels at 1 024 factors on the same triplets (scripts/kahfm_bench.py's measurement)
  slope      el_slope_scores for all users on the same matrix with ratings 1..5
Recorded, not gated.  One JSON line on stdout, appended to profiles/bprslim_bench.jsonl.

Usage:  python scripts/bprslim_bench.py [--reps 3] [--skip kahfm,slope]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr  # noqa: E402

INFINITY_CACHE_GATHER_TBS = 8.6
U, I = 6040, 3706
LR, LI_REG, LJ_REG = 0.05, 0.1, 0.001


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


def wall_s(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return sorted(out)[reps // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bprslim_bench"))
    a = ap.parse_args()
    skip = set(a.skip.split(",")) if a.skip else set()
    ctx = ops.get_context(0)
    dev = ctx.device
    ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
    n = int(ix.shape[0])
    R = sp.csr_matrix((np.ones(n), ix, ip), shape=(U, I))
    pos = ops.DeviceCSR(ip, ix, I, dev)
    u, i, j = (x.cpu().numpy() for x in ops.bpr_sample(ctx, pos, n, seed=42))
    t0 = time.perf_counter()
    order, starts = ops.bprslim_levels(i, j, I)
    schedule_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    sgd_order, sgd_starts = ops.sgd_levels(u, i, j, U, I)
    sgd_schedule_s = time.perf_counter() - t0
    sizes = np.diff(starts)
    st = ops.BprSlimDeviceState(ctx, R, LR, LI_REG, LJ_REG)
    du, di, dj = (torch.from_numpy(np.ascontiguousarray(x[order], dtype=np.int32)).to(dev) for x in (u, i, j))
    x_dev = torch.empty(n, dtype=torch.float64, device=dev)

    def epoch():
        ops.bprslim_apply(ctx, du, di, dj, st.rows, st.S, LR, LI_REG, LJ_REG, x_out=x_dev, level_start=starts)
    epoch()                                                       # warm-up epoch (first launches)
    epoch_s, epoch_runs = wall_s(epoch, a.reps)
    ctx.timing_report()
    ctx.timing(True)
    try:
        epoch()
        torch.cuda.synchronize()
    finally:
        ctx.timing(False)
    launches, kernel_ms = ctx.timing_report()["k_bprslim_apply"][:2]
    seen = float(np.diff(ip)[u].sum())                            # seen items over the epoch's triplets
    St = ops.bprslim_table(ctx, st.S)
    table_ms = median(lambda: ops.bprslim_table(ctx, st.S, out=St), a.reps)
    P = torch.empty((st.block_rows, I), dtype=torch.float64, device=dev)

    def scores():
        for s in range(0, U, st.block_rows):
            ops.bprslim_scores(ctx, st.rows, St, s, min(s + st.block_rows, U), out=P)
    scores()
    scores_ms = median(scores, a.reps)
    del P
    st.recommend(("excl", pos), 10, 0, 256)
    rec_ms = median(lambda: st.recommend(("excl", pos), 10, 0, U), a.reps)
    st_bytes = float(n) * I * 8.0
    line = {"users": U, "items": I, "nnz": n, "triplets": n, "levels": int(len(sizes)), "level_mean": round(float(sizes.mean()), 1),
            "level_largest": int(sizes.max()), "schedule_host_s": round(schedule_s, 4),
            "bprsgd_levels_same_triplets": int(len(sgd_starts) - 1), "bprsgd_schedule_host_s": round(sgd_schedule_s, 4),
            "epoch_wall_s_median": round(epoch_s, 4), "epoch_wall_s_runs": [round(x, 4) for x in epoch_runs],
            "us_per_level": round(epoch_s / len(sizes) * 1e6, 2), "epoch_launches": int(launches),
            "epoch_kernels_s": round(kernel_ms / 1e3, 4), "seen_items_per_triplet": round(seen / n, 1),
            "s_bytes_per_epoch": 48.0 * seen, "s_GBps_over_wall": round(48.0 * seen / epoch_s / 1e9, 1),
            "table_ms": round(table_ms, 3), "scores_ms": round(scores_ms, 3),
            "st_read_tb_per_s": round(st_bytes / scores_ms / 1e9, 3),
            "pct_of_infinity_cache_gather": round(100.0 * st_bytes / scores_ms / 1e9 / INFINITY_CACHE_GATHER_TBS, 1),
            "recommend_ms": round(rec_ms, 3), "recommend_users_per_s": round(U / rec_ms * 1e3, 1), "device": ctx.arch}
    del st, St
    torch.cuda.empty_cache()
    if "slope" not in skip:
        rs = np.random.RandomState(3)
        Rr = sp.csr_matrix((rs.randint(1, 6, n).astype(np.float64), ix, ip), shape=(U, I))
        sl = ops.SlopeDeviceState(ctx, Rr, (ip, ix))
        sl.build()
        P = torch.empty((sl.block_rows, I), dtype=torch.float64, device=dev)

        def slope_scores():
            for s in range(0, U, sl.block_rows):
                ops.slope_scores(ctx, sl.rows, sl.user_mean, sl.T, s, min(s + sl.block_rows, U), out=P)
        slope_scores()
        line["slope_scores_ms"] = round(median(slope_scores, a.reps), 3)
        del sl, P
        torch.cuda.empty_cache()
    if "kahfm" not in skip:
        from attr_bench import item_features
        nF = 1024
        F, w = item_features(I, nF, 20, seed=4)
        P0, Q0 = ops.kahfm_init(ctx, ip, ix, F, w)
        ks = ops.BprSgdDeviceState(ctx, P0, Q0, torch.zeros(I, dtype=torch.float64, device=dev), lr=0.05, reg_bias=0.0,
                                   reg_user=0.0025, reg_pos=0.0025, reg_neg=0.00025)
        ku, ki, kj = (torch.from_numpy(np.ascontiguousarray(x[sgd_order], dtype=np.int32)).to(dev) for x in (u, i, j))
        k_levels = int(len(sgd_starts) - 1)

        def kahfm_epoch():
            ops.check(ctx.lib.el_bprsgd_apply_levels(ctx.handle, ctx.stream(), C.byref(ks._c), ops._ptr(ku), ops._ptr(ki),
                                                     ops._ptr(kj), sgd_starts.ctypes.data_as(C.c_void_p), k_levels),
                      "el_bprsgd_apply_levels")
        kahfm_epoch()
        k_s, k_runs = wall_s(kahfm_epoch, a.reps)
        line.update(kahfm_features=nF, kahfm_levels=k_levels, kahfm_epoch_wall_s_median=round(k_s, 4),
                    kahfm_epoch_wall_s_runs=[round(x, 4) for x in k_runs])
    print(json.dumps(line), flush=True)
    with open(a.out + ".jsonl", "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
