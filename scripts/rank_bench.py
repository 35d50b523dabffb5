"""Time the rank pass (el_score_rank, both routes), el_rank_metrics and el_score_topk (k = 10) on the same block in one run.

Shapes: ml1m = 6040 x 3706, F = 64; c2 = one 131 072-user block of the second benchmark configuration (100 000 items, F = 128).
Profiles are Zipf (elliot_amd.synthetic.zipf_csr); a random 20 % of every profile is held out, the rest is the exclusion mask.
Medians of 3 after one warm-up, every pass on the whole block.

Run:  python scripts/rank_bench.py [--shapes ml1m,c2] [--out results/rank_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elliot_amd import ops                                   # noqa: E402
from elliot_amd.synthetic import zipf_csr                    # noqa: E402

SHAPES = {"ml1m": dict(U=6040, I=3706, F=64, zipf=dict(mean_log=4.5, sigma_log=1.0, dmin=20, dmax=3000, seed=5)),
          "c2": dict(U=131072, I=100000, F=128, zipf=dict(mean_log=3.9, sigma_log=1.0, dmin=5, dmax=2000, seed=1234))}


def split(indptr, indices, ratio, seed):
    rs = np.random.RandomState(seed)
    held = rs.rand(indices.shape[0]) < ratio
    rows = np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr))
    out = []
    for keep in (~held, held):
        p = np.zeros(indptr.shape[0], dtype=np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=indptr.shape[0] - 1), out=p[1:])
        out.append((p, indices[keep].astype(np.int32)))
    return out


def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def run(ctx, name, U, I, F, zipf):
    indptr, indices = zipf_csr(U, I, **zipf)
    (trp, tri), (tep, tei) = split(indptr, indices, 0.2, 7)
    train = ops.DeviceCSR(trp, tri, I, ctx.device)
    test = ops.DeviceTestSet(tep, tei, None, ctx.device)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(3)
    Gu = torch.randn((U, F), generator=g, device=ctx.device) * 0.1
    Gi = torch.randn((I, F), generator=g, device=ctx.device) * 0.1
    Bi = torch.randn(I, generator=g, device=ctx.device) * 0.01
    held = np.diff(tep)
    res = {"shape": name, "users": U, "items": I, "F": F, "held_out": int(tei.shape[0]), "held_out_mean": float(held.mean()),
           "users_over_mfma_cap": int((held > ops.RANK_MFMA_CAP).sum()), "train_nnz": int(tri.shape[0])}
    pos = {}

    def rank(algo, stop=U):
        pos[algo] = ops.score_rank(ctx, Gu, Gi, Bi, 0, stop, test, excl=train, algo=algo)
    res["rank_mfma_ms"] = timed(lambda: rank("mfma"))
    res["rank_wave_ms"] = timed(lambda: rank("simple"))
    res["routes_agree"] = bool(torch.equal(pos["mfma"], pos["simple"]))
    ctx.timing(True)
    rank("auto", min(U, 256))
    res["auto_route"] = "mfma" if "k_score_rank_mfma" in ctx.timing_report() else "wave"
    ctx.timing(False)
    res["topk_ms"] = timed(lambda: ops.score_topk(ctx, Gu, Gi, Bi, 0, U, 10, excl=train))
    res["rank_metrics_ms"] = timed(lambda: ops.rank_metrics(ctx, pos["mfma"], test, 0.0, train, I, 10))
    res["rank_mfma_over_topk"] = res["rank_mfma_ms"] / res["topk_ms"]
    res["rank_wave_us_per_user"] = 1e3 * res["rank_wave_ms"] / U
    res["rank_mfma_us_per_user"] = 1e3 * res["rank_mfma_ms"] / U
    sums = ops.rank_metrics(ctx, pos["mfma"], test, 0.0, train, I, 10).cpu().numpy()
    res["AUC"] = float(sums[0] / sums[1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,c2")
    ap.add_argument("--out", default="results/rank_bench.json")
    args = ap.parse_args()
    ctx = ops.get_context(0)
    out = []
    for name in args.shapes.split(","):
        r = run(ctx, name, **SHAPES[name])
        print(json.dumps(r), flush=True)
        out.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
