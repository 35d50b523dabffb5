"""Time the beyond-accuracy metric passes against the accuracy kernel on one evaluation block (needs the GPU).

Per block of 131 072 users x 10 list entries, at I = 100 K and I = 1 M items, for three kinds of lists (uniform ids, Zipf ids, one
identical list for everyone), cutoff 10:
  el_rec_metrics                        the accuracy kernel alone (what an evaluation cost before), measured in the same run
  el_beyond_metrics                     the per-user pass + histogram, tile-aggregated adds (the default) and EL_BEYOND_HIST_DIRECT
  el_beyond_hist_finish                 radix sort of the counts, n / free / G, nov
  el_beyond_entropy                     the second pass over the lists
Each figure is the median over --reps calls of a device-event interval around ONE call, after --warmup calls; the forms alternate
inside one repetition.  Writes a markdown table (stdout, and --out FILE).

Run:  python scripts/metrics_bench.py [--reps 20] [--warmup 3] [--out profiles/metrics_beyond_bench.md] [--users 131072]

--fair times the fairness passes instead (el_metrics_fair.hip), on the Zipf block at I = 1 M with 2 and with 16 user / item groups:
  el_fair_metrics + el_group_sums       the per-block pass (ops.fair_metrics), without and with the lists' scores
  el_fair_item_finish                   the per-item pass after the last block
  el_rec_metrics, el_beyond_metrics     on the same block in the same run, the yardsticks
Run:  python scripts/metrics_bench.py --fair [--out profiles/metrics_fair_bench.md]
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from elliot_amd import ops  # noqa: E402
from elliot_amd.evaluation import beyond  # noqa: E402

K, CUTOFF, THR = 10, 10, 3.0


def zipf_ids(rs, I, size, a=1.0):
    cdf = np.cumsum(1.0 / np.arange(1, I + 1) ** a)
    cdf /= cdf[-1]
    return rs.permutation(I)[np.searchsorted(cdf, rs.rand(*size)).clip(0, I - 1)].astype(np.int32)


def rows_csr(rs, U, I, per_row):
    cols = np.sort(rs.randint(0, I, size=(U, per_row)), axis=1).astype(np.int32)      # (duplicates inside a row are harmless for timing)
    return np.arange(0, U * per_row + 1, per_row, dtype=np.int64), cols.reshape(-1)


def timed(fns, reps, warmup):
    """{name: (median, min, max) ms}: the forms alternate inside each repetition"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
    return {name: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for name, v in out.items()}


def fair_leg(ctx, args):
    from elliot_amd.evaluation import fairness
    U, I = args.users, 1_000_000
    rs = np.random.RandomState(I % 1000)
    qp, qc = rows_csr(rs, U, I, 20)
    tp, tc = rows_csr(rs, U, I, 5)
    tr = rs.randint(1, 6, size=tc.shape[0]).astype(np.float32)
    m = sp.csr_matrix((np.ones(qc.shape[0], np.float32), qc, qp), shape=(U, I))
    m.sum_duplicates()
    m.sort_indices()
    tables = ops.DeviceItemTables(beyond.ItemTables(m, int(m.nnz), U), ctx.device)
    train = ops.DeviceCSR(m.indptr, m.indices, I, ctx.device)
    test = ops.DeviceTestSet(tp, tc, tr, ctx.device)
    cols = ops.DeviceTestColumns(tp, tc, I, ctx.device)
    lists = zipf_ids(rs, I, (U, K))
    idx = torch.from_numpy(np.ascontiguousarray(lists)).to(ctx.device)
    val = torch.from_numpy(rs.rand(U, K).astype(np.float32)).to(ctx.device)
    acc = torch.zeros(8, dtype=torch.float64, device=ctx.device)
    sums = torch.zeros(ops.BEYOND_SUMS, dtype=torch.float64, device=ctx.device)
    hist = torch.zeros(I, dtype=torch.int32, device=ctx.device)
    lines = ["| groups | el_rec_metrics | el_beyond_metrics | fairness pass per block | the same with scores | el_fair_item_finish |",
             "|---|---|---|---|---|---|"]
    for G in (2, 16):
        def grouping(n):
            lab = rs.randint(0, G, size=n)
            return ops.DeviceGrouping(fairness.Grouping(lab, G, np.bincount(lab, minlength=G), n, "bench"), ctx.device)
        items, users = grouping(I), grouping(U)
        state = ops.FairState(ctx, test, I, items, users)
        fns = {"rec": lambda: ops.rec_metrics(ctx, idx, test, THR, CUTOFF, sums=acc),
               "beyond": lambda: ops.beyond_metrics(ctx, idx, test, train, tables, THR, CUTOFF, sums=sums, hist=hist),
               "fair": lambda: ops.fair_metrics(ctx, idx, None, test, train, items, users, THR, CUTOFF, I, state),
               "scores": lambda: ops.fair_metrics(ctx, idx, val, test, train, items, users, THR, CUTOFF, I, state),
               "finish": lambda: ops.fair_item_finish(ctx, test, cols, items, THR, state)}
        t = timed(fns, args.reps, args.warmup)
        lines.append(f"| {G} x {G} | " + " | ".join(f"{t[n][0]:.3f} ms ({t[n][1]:.3f}-{t[n][2]:.3f})" for n in fns) + " |")
        print(lines[-1], flush=True)
    return (f"Block of {U} users x {K} list entries (Zipf ids), I = {I}, cutoff {CUTOFF}, threshold {THR}; median (min-max) of {args.reps} "
            f"device-event intervals around one call each, {args.warmup} warm-up calls; {ctx.arch}.\n\n" + "\n".join(lines) + "\n")


def write_out(args, text):
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--items", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--out", default=None)
    ap.add_argument("--fair", action="store_true", help="time the fairness passes instead")
    args = ap.parse_args()
    ctx = ops.get_context(0)
    if args.fair:
        return write_out(args, fair_leg(ctx, args))
    U = args.users
    lines = [f"| I | lists | el_rec_metrics | el_beyond_metrics (tile-aggregated) | el_beyond_metrics (direct adds) | el_beyond_hist_finish | "
             f"el_beyond_entropy | new passes together (default form) |", "|---|---|---|---|---|---|---|---|"]
    for I in args.items:
        rs = np.random.RandomState(I % 1000)
        qp, qc = rows_csr(rs, U, I, 20)
        tp, tc = rows_csr(rs, U, I, 5)
        tr = rs.randint(1, 6, size=tc.shape[0]).astype(np.float32)
        m = sp.csr_matrix((np.ones(qc.shape[0], np.float32), qc, qp), shape=(U, I))
        m.sum_duplicates()
        m.sort_indices()
        tables = ops.DeviceItemTables(beyond.ItemTables(m, int(m.nnz), U), ctx.device)
        train = ops.DeviceCSR(m.indptr, m.indices, I, ctx.device)
        test = ops.DeviceTestSet(tp, tc, tr, ctx.device)
        kinds = {"uniform": rs.randint(0, I, size=(U, K)).astype(np.int32), "zipf": zipf_ids(rs, I, (U, K)),
                 "identical": np.tile(rs.choice(I, K, replace=False).astype(np.int32), (U, 1))}
        for kind, lists in kinds.items():
            idx = torch.from_numpy(np.ascontiguousarray(lists)).to(ctx.device)
            acc = torch.zeros(8, dtype=torch.float64, device=ctx.device)
            sums = torch.zeros(ops.BEYOND_SUMS, dtype=torch.float64, device=ctx.device)
            hist = torch.zeros(I, dtype=torch.int32, device=ctx.device)
            ent = torch.zeros(1, dtype=torch.float64, device=ctx.device)
            ops.beyond_metrics(ctx, idx, test, train, tables, THR, CUTOFF, sums=sums, hist=hist)
            _, nov = ops.beyond_hist_finish(ctx, hist)
            fns = {"rec": lambda: ops.rec_metrics(ctx, idx, test, THR, CUTOFF, sums=acc),
                   "agg": lambda: ops.beyond_metrics(ctx, idx, test, train, tables, THR, CUTOFF, sums=sums, hist=hist),
                   "direct": lambda: ops.beyond_metrics(ctx, idx, test, train, tables, THR, CUTOFF, sums=sums, hist=hist, direct=True),
                   "finish": lambda: ops.beyond_hist_finish(ctx, hist),
                   "entropy": lambda: ops.beyond_entropy(ctx, idx, test, nov, CUTOFF, total=ent)}
            t = timed(fns, args.reps, args.warmup)
            cell = lambda n: f"{t[n][0]:.3f} ms ({t[n][1]:.3f}-{t[n][2]:.3f})"          # noqa: E731
            together = t["agg"][0] + t["finish"][0] + t["entropy"][0]
            lines.append(f"| {I} | {kind} | {cell('rec')} | {cell('agg')} | {cell('direct')} | {cell('finish')} | {cell('entropy')} | "
                         f"{together:.3f} ms |")
            print(lines[-1], flush=True)
    text = (f"Block of {U} users x {K} list entries, cutoff {CUTOFF}, threshold {THR}; median (min-max) of {args.reps} device-event "
            f"intervals around one call each, {args.warmup} warm-up calls; {ctx.arch}.\n\n" + "\n".join(lines) + "\n")
    write_out(args, text)


if __name__ == "__main__":
    main()
