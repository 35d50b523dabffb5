"""Time PureSVD on the device: the pattern's host transposition and upload, the build by stage (start-matrix draw, the
2 n_iter + 2 products, the 2 n_iter + 1 orthonormalisations, Gram + eigh, projection + signs, and the rest: the start matrix's
upload and the small copies) and every user's top-10; medians of 3 after a warm-up.  The stages are timed from here, by wrapping
the public functions of ops that build() calls with a synchronised clock; build() itself carries no instrumentation.
Beside them the kernels alone (hipEvents): one product per orientation with its gather rate nnz x R x 8 B / time, the Gram with
its fp64 FLOP rate 2 n R^2 / time, one orthonormalisation.

  ml1m     an ML-1M-shaped synthetic pattern (6 040 x 3 706, ~1 M entries: slim_bench.py's generator), factors 50
  c2       configs[1] of bench.py: 1 M x 100 K, ~78 M entries (als_bench.py's generator), factors 50

One JSON line per leg on stdout.  Usage:  python scripts/puresvd_bench.py [--legs ml1m,c2] [--factors 50] [--k 10]
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

SEED = 42
SPMM_F32_GATHER_TBS = 7.4        # k_spmm_csr's recorded fp32 gather rate (README, round-6 table): context, not a gate


def timed(fn, reps=3):
    """(median ms, all ms) of `reps` runs bracketed by events on the current stream."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(x, 3) for x in ms]


def top10_all(st, excl, k, block=65536):
    for s in range(0, st.U, block):
        st.recommend(("excl", excl), k, s, min(s + block, st.U))


STAGES = {"psvd_start_matrix": "draw", "spmm_csr_f64": "spmm", "psvd_orth": "orth", "gram_f64": "gram_eigh",
          "psvd_small_svd": "gram_eigh", "psvd_project": "project", "psvd_signs": "project"}


class StageClock:
    """While active, every function of ops named in STAGES runs between two synchronisations and adds its wall time to its stage."""

    def __init__(self):
        self.ms = {stage: 0.0 for stage in STAGES.values()}
        self.calls = {name: 0 for name in STAGES}

    def wrap(self, name, fn):
        def clocked(*args, **kwargs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kwargs)
            torch.cuda.synchronize()
            self.ms[STAGES[name]] += 1e3 * (time.perf_counter() - t0)
            self.calls[name] += 1
            return out
        return clocked

    def __enter__(self):
        self.saved = {name: getattr(ops, name) for name in STAGES}
        for name, fn in self.saved.items():
            setattr(ops, name, self.wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(ops, name, fn)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def run_leg(ctx, leg, ip, ix, U, I, factors, k, reps=3):
    A = sp.csr_matrix((np.ones(ix.shape[0], np.float32), ix, ip), shape=(U, I))
    stages, totals, uploads = [], [], []
    for rep in range(reps + 1):                                  # the first run is the warm-up
        st = ops.PureSvdDeviceState(ctx, A, factors, SEED)
        upload = wall_ms(st.upload)                              # host transposition + both orientations to the device
        with StageClock() as clock:
            total = wall_ms(st.build)
        if rep:
            uploads.append(upload)
            totals.append(total)
            stages.append(dict(clock.ms, other=total - sum(clock.ms.values()), n_spmm=clock.calls["spmm_csr_f64"],
                               n_orth=clock.calls["psvd_orth"]))
    med = {key: round(float(np.median([s[key] for s in stages])), 3) for key in stages[0]}
    upload_ms = float(np.median(uploads))
    M, Mt = st.upload()                                          # build() released the pattern: once more, for the kernels alone
    R = st.R
    X = torch.from_numpy(ops.psvd_start_matrix(M.n_cols, R, SEED)).to(ctx.device)
    Y = torch.empty((M.n_rows, R), dtype=torch.float64, device=ctx.device)
    fwd_ms, fwd_all = timed(lambda: ops.spmm_csr_f64(ctx, M, X, out=Y, holder=st, verify=False))
    back = torch.empty((M.n_cols, R), dtype=torch.float64, device=ctx.device)
    bwd_ms, bwd_all = timed(lambda: ops.spmm_csr_f64(ctx, Mt, Y, out=back, holder=st, verify=False))
    gram_ms, gram_all = timed(lambda: ops.gram_f64(ctx, Y, holder=st))
    orth_ms, orth_all = timed(lambda: ops.psvd_orth(ctx, Y, holder=st))
    excl = ops.DeviceCSR(A.indptr, A.indices, I, ctx.device)
    top10_all(st, excl, k)
    score_ms, score_all = timed(lambda: top10_all(st, excl, k))
    gather = lambda ms: round(A.nnz * R * 8 / (ms / 1e3) / 1e12, 3)
    line = {"leg": leg, "model": "PureSVD", "users": int(U), "items": int(I), "nnz": int(A.nnz), "factors": factors, "R": R,
            "n_iter": st.n_iter, "transposed": bool(st.transposed), "k": k,
            "build_ms_median": round(float(np.median(totals)), 2), "build_ms_runs": [round(t, 2) for t in totals],
            "upload_pattern_ms_median": round(upload_ms, 2), "upload_pattern_ms_runs": [round(t, 2) for t in uploads],
            "cold_build_ms_median": round(upload_ms + float(np.median(totals)), 2), "stage_ms_median": med,
            "spmm_M_ms_median": round(fwd_ms, 4), "spmm_M_ms_runs": fwd_all, "spmm_M_gather_TBps": gather(fwd_ms),
            "spmm_Mt_ms_median": round(bwd_ms, 4), "spmm_Mt_ms_runs": bwd_all, "spmm_Mt_gather_TBps": gather(bwd_ms),
            "spmm_f32_gather_TBps_recorded": SPMM_F32_GATHER_TBS,
            "long_rows": [M.n_long, Mt.n_long], "pieces": [M.n_pieces, Mt.n_pieces],
            "gram_ms_median": round(gram_ms, 4), "gram_ms_runs": gram_all, "gram_rows": int(M.n_rows),
            "gram_fp64_TFLOPs": round(2.0 * M.n_rows * R * R / (gram_ms / 1e3) / 1e12, 4),
            "orth_ms_median": round(orth_ms, 4), "orth_ms_runs": orth_all,
            "score_topk_all_users_ms_median": round(score_ms, 3), "score_ms_runs": score_all,
            "users_per_s": round(U / (score_ms / 1e3)), "device": ctx.arch}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ml1m,c2")
    ap.add_argument("--factors", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    ctx = ops.get_context(0)
    if "ml1m" in legs:
        U, I = 6040, 3706
        ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
        run_leg(ctx, "ml1m", ip, ix, U, I, args.factors, args.k)
    if "c2" in legs:
        U, I = 1000000, 100000
        ip, ix = zipf_csr_device(U, I, ctx.device, mean_log=3.9, sigma_log=1.0, dmin=5, dmax=2000, seed=1234)
        ip, ix = ip.cpu().numpy(), ix.cpu().numpy()
        run_leg(ctx, "c2", ip, ix, U, I, args.factors, args.k)


if __name__ == "__main__":
    main()
