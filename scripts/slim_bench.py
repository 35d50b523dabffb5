"""Time the SLIM kernels at the ML-1M shape: el_slim_order, el_slim_fit over every column, el_slim_w, and every user's top-10
(el_knn_score_topk on the built W); hipEvents, medians of 3 after a warm-up.

  ml1m     an ML-1M-shaped synthetic set (6 040 x 3 706, ~1 M integer ratings 1-5: rp3_bench.py's generator)

for the reference's default hyper-parameters (alpha = l1_ratio = 0.001) and for alpha 0.01, l1_ratio 0.1.  Beside the times the
line reports what the solver did: sweeps (mean / max over the columns), coordinate steps (a step = one draw whose column has a
non-zero norm) and non-zero visits (the entries of the visited columns: every one is gathered once for the dot and touched by up to
two residual updates) per second, and, since a target is one sequential chain, the time per coordinate step of the
longest-running target -- fitted alone, [j, j + 1) -- which is the latency of one step.  One JSON line per parameter set on stdout.

Usage:  python scripts/slim_bench.py [--neighbors 10] [--k 10] [--params 0.001:0.001,0.01:0.1]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr  # noqa: E402

SEED = 42


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


def run(ctx, R, alpha, l1_ratio, N, k):
    U, I = R.shape
    Rd = ops.DeviceCSR(R.indptr, R.indices, I, ctx.device)
    Rv = ops.device_values(R.data, ctx.device)
    csc, vals = ops.slim_csc(ctx, R)
    n_draws = ops.SLIM_MAX_ITER * I
    state = ops.slim_seed_state(SEED)
    order = ops.slim_order(ctx, state, I, n_draws)               # warm-up of every stage
    lists = ops.slim_fit(ctx, csc, vals, alpha, l1_ratio, order, N)
    W, Wv = ops.slim_w(ctx, *lists[:3])
    ops.knn_score_topk(ctx, Rd, Rv, W, Wv, 0, min(U, 1024), k, excl=Rd)
    torch.cuda.synchronize()
    order_ms, order_all, order = timed(lambda: ops.slim_order(ctx, state, I, n_draws))
    fit_ms, fit_all, lists = timed(lambda: ops.slim_fit(ctx, csc, vals, alpha, l1_ratio, order, N))
    w_ms, w_all, (W, Wv) = timed(lambda: ops.slim_w(ctx, *lists[:3]))
    score_ms, score_all, _ = timed(lambda: ops.knn_score_topk(ctx, Rd, Rv, W, Wv, 0, U, k, excl=Rd))
    n_iter = lists[3].cpu().numpy().astype(np.int64)
    # the work of the call, recounted on the host from the visiting order and the sweeps every column ran
    col_nnz = np.diff(csc.indptr.cpu().numpy())
    visit = order.cpu().numpy()
    live = (col_nnz[visit] > 0).astype(np.int64)
    steps_after = np.concatenate([[0], np.cumsum(live.reshape(ops.SLIM_MAX_ITER, I).sum(1))])
    nnz_after = np.concatenate([[0], np.cumsum(col_nnz[visit].reshape(ops.SLIM_MAX_ITER, I).sum(1))])
    steps, visits = int(steps_after[n_iter].sum()), int(nnz_after[n_iter].sum())
    slow = int(np.argmax(nnz_after[n_iter] + 64 * steps_after[n_iter]))
    one_ms, one_all, _ = timed(lambda: ops.slim_fit(ctx, csc, vals, alpha, l1_ratio, order, N, slow, slow + 1))
    line = {"leg": "ml1m", "model": "Slim", "users": int(U), "items": int(I), "ratings": int(R.nnz), "alpha": alpha,
            "l1_ratio": l1_ratio, "neighborhood": N, "k": k, "exclusion": "column",
            "order_ms_median": round(order_ms, 3), "order_ms_runs": order_all, "order_draws": n_draws,
            "fit_ms_median": round(fit_ms, 1), "fit_ms_runs": fit_all,
            "sweeps_mean": round(float(n_iter.mean()), 2), "sweeps_max": int(n_iter.max()),
            "columns_out_of_sweeps": int((n_iter == ops.SLIM_MAX_ITER).sum()),
            "coordinate_steps": steps, "coordinate_steps_per_s": round(steps / (fit_ms / 1e3)),
            "nonzero_visits": visits, "nonzero_visits_per_s": round(visits / (fit_ms / 1e3)),
            "slim_w_ms_median": round(w_ms, 3), "slim_w_ms_runs": w_all, "W_nnz": int(W.nnz),
            "score_topk_all_users_ms_median": round(score_ms, 3), "score_ms_runs": score_all,
            "users_per_s": round(U / (score_ms / 1e3)),
            "longest_target": slow, "longest_target_sweeps": int(n_iter[slow]), "longest_target_steps": int(steps_after[n_iter[slow]]),
            "longest_target_alone_ms_median": round(one_ms, 2), "longest_target_ms_runs": one_all,
            "longest_target_us_per_step": round(one_ms * 1e3 / max(int(steps_after[n_iter[slow]]), 1), 3),
            "longest_target_nonzeros_per_step": round(float(nnz_after[n_iter[slow]]) / max(int(steps_after[n_iter[slow]]), 1), 1),
            "device": ctx.arch}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--neighbors", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--params", default="0.001:0.001,0.01:0.1")
    args = ap.parse_args()
    ctx = ops.get_context(0)
    U, I = 6040, 3706
    ip, ix = zipf_csr(U, I, mean_log=4.75, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.8, seed=3)
    rs = np.random.RandomState(3)
    R = sp.csr_matrix((rs.randint(1, 6, size=ix.shape[0]).astype(np.float32), ix, ip), shape=(U, I))
    for pair in args.params.split(","):
        alpha, l1_ratio = (float(x) for x in pair.split(":"))
        run(ctx, R, alpha, l1_ratio, args.neighbors, args.k)


if __name__ == "__main__":
    main()
