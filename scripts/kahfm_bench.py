"""Time KaHFM's device side at the ML-1M shape for several feature counts: el_kahfm_init, one epoch of el_bprsgd_apply_levels on
wide rows (k_bprsgd_apply_wide) and el_score_topk_f64 for all users.

  ratings    ML-1M-shaped synthetic ratings (6 040 x 3 706, ~1 M; zipf_csr with the parameters of scripts/attr_bench.py)
  features   the reference's knowledge-graph files for ML-1M are not distributed with it, so the statistics are ASSUMED:
             --per-item 20 Zipf-distributed features per item on average (1 .. 2 x per-item) out of nF, TF-IDF weights replaced by
             uniform (0, 1] doubles (the kernels do not care)
  triplets   one epoch = as many Philox triplets as ratings (el_bpr_sample), level-scheduled on the host (el_bprsgd_levels_host)

Per nF one JSON line: levels, the host time of the schedule, the wall time of the epoch's launches (launch .. synchronize, without
event brackets), the summed hipEvent brackets of the kernels in a second epoch, the bytes the kernel moves per triplet (three rows
read and written: 48 nF; the two-pass shape above 4 096 factors reads them twice: 72 nF) and the rate that makes, and the time of
el_score_topk_f64 over all users (k = 10, train items excluded).

--reference <checkout>: also the reference's own KAHFMModel.update_factors (kahfm_model.py, loaded by file path, NumPy on the
CPU of the machine this runs on) on --reference-triplets random triplets at every nF, seconds per triplet.  No GPU is needed for
that part alone (--legs reference).

Usage:  python scripts/kahfm_bench.py [--features 1024,4096,8192] [--per-item 20] [--legs gpu,reference] [--reference PATH]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12            # MI355X: 8 TB/s
U, I = 6040, 3706
HP = dict(lr=0.05, reg_bias=0.0, reg_user=0.0025, reg_pos=0.0025, reg_neg=0.00025)


def reference_leg(path, widths, n):
    spec = importlib.util.spec_from_file_location(
        "kahfm_model", os.path.join(path, "elliot", "recommender", "knowledge_aware", "kaHFM", "kahfm_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    rs = np.random.RandomState(0)
    for nF in widths:
        m = object.__new__(mod.KAHFMModel)
        m._global_bias, m._item_bias = 0, np.zeros(I)
        m._user_factors, m._item_factors = rs.uniform(0, 0.05, size=(U, nF)), rs.uniform(0, 0.3, size=(I, nF))
        m._learning_rate, m._bias_regularization, m._user_regularization = HP["lr"], HP["reg_bias"], HP["reg_user"]
        m._positive_item_regularization, m._negative_item_regularization = HP["reg_pos"], HP["reg_neg"]
        u, i, j = rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, I, n)
        for t in range(200):                                      # warm-up
            m.update_factors(u[t], i[t], j[t])
        t0 = time.perf_counter()
        for t in range(n):
            m.update_factors(u[t], i[t], j[t])
        dt = (time.perf_counter() - t0) / n
        print(json.dumps({"leg": "reference", "what": "KAHFMModel.update_factors, NumPy on this machine's CPU", "features": nF,
                          "triplets": n, "seconds_per_triplet": dt, "seconds_per_1M_triplets": round(dt * 1e6, 1)}), flush=True)


def gpu_leg(widths, per_item):
    import torch
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    from attr_bench import item_features
    ctx = ops.get_context(0)
    dev = ctx.device
    ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
    pos = ops.DeviceCSR(ip, ix, I, dev)
    n = int(ix.shape[0])
    u, i, j = (x.cpu().numpy() for x in ops.bpr_sample(ctx, pos, n, seed=42))
    t0 = time.perf_counter()
    order, starts = ops.sgd_levels(u, i, j, U, I)
    schedule_s = time.perf_counter() - t0
    levels = int(starts.shape[0] - 1)
    du, di, dj = (torch.from_numpy(np.ascontiguousarray(x[order], dtype=np.int32)).to(dev) for x in (u, i, j))
    import ctypes as C

    def epoch(st):
        ops.check(ctx.lib.el_bprsgd_apply_levels(ctx.handle, ctx.stream(), C.byref(st._c), ops._ptr(du), ops._ptr(di), ops._ptr(dj),
                                                 starts.ctypes.data_as(C.c_void_p), levels), "el_bprsgd_apply_levels")
        torch.cuda.synchronize()

    for nF in widths:
        F, w = item_features(I, nF, per_item, seed=4)
        ctx.timing(True)
        P0, Q0 = ops.kahfm_init(ctx, ip, ix, F, w)
        init = ctx.timing_report()
        ctx.timing(False)
        st = ops.BprSgdDeviceState(ctx, P0, Q0, torch.zeros(I, dtype=torch.float64, device=dev), **HP)
        del P0, Q0
        epoch(st)                                                 # warm-up epoch (first launches)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            epoch(st)
            walls.append(time.perf_counter() - t0)
        ctx.timing(True)
        epoch(st)
        rep = ctx.timing_report()
        ctx.timing(False)
        kern = {k: v for k, v in rep.items() if k.startswith("k_bprsgd")}
        kernel_s = sum(v[1] for v in kern.values()) / 1e3
        scores = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.score_topk_f64(ctx, st.P, st.Q, st.b, 0, U, 10, excl=pos)
            torch.cuda.synchronize()
            scores.append(time.perf_counter() - t0)
        bytes_per_triplet = (72 if nF > 4096 else 48) * nF
        wall = sorted(walls)[1]
        print(json.dumps({
            "leg": "gpu", "users": U, "items": I, "features": nF, "item_feature_nnz": int(F.nnz), "triplets": n, "levels": levels,
            "largest_level": int(np.diff(starts).max()), "schedule_host_s": round(schedule_s, 3),
            "epoch_wall_s_median": round(wall, 4), "epoch_wall_s_runs": [round(x, 4) for x in walls],
            "epoch_kernels_s": round(kernel_s, 4), "kernels": {k: [v[0], round(v[1], 2)] for k, v in kern.items()},
            "bytes_per_triplet": bytes_per_triplet, "GBps_over_wall": round(bytes_per_triplet * n / wall / 1e9, 1),
            "GBps_over_kernels": round(bytes_per_triplet * n / kernel_s / 1e9, 1),
            "share_of_hbm_peak_over_kernels": round(bytes_per_triplet * n / kernel_s / HBM_PEAK, 3),
            "kahfm_init_ms": {k: round(v[1], 3) for k, v in init.items()},
            "score_topk_f64_all_users_s_median": round(sorted(scores)[1], 4), "score_topk_f64_s_runs": [round(x, 4) for x in scores],
            "device": ctx.arch}), flush=True)
        del st
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="1024,4096,8192")
    ap.add_argument("--per-item", type=int, default=20)
    ap.add_argument("--legs", default="gpu")
    ap.add_argument("--reference", default=os.environ.get("ELLIOT_REF"))
    ap.add_argument("--reference-triplets", type=int, default=20000)
    args = ap.parse_args()
    widths = [int(x) for x in args.features.split(",")]
    legs = args.legs.split(",")
    if "reference" in legs:
        if not args.reference:
            raise SystemExit("--legs reference needs --reference <checkout> (or $ELLIOT_REF)")
        reference_leg(args.reference, widths, args.reference_triplets)
    if "gpu" in legs:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        gpu_leg(widths, args.per_item)


if __name__ == "__main__":
    main()
