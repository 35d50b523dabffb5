"""DMF on one MI355X: a DMF step (el_dmf_train_step, cosine / reference) beside, in the same process and on the same samples, the FISM
and NAIS steps (F = 64); the Adam-fused first-layer fan-out as bytes over time against its floor; one full evaluation (towers of all
rows, then el_dmf_scores + el_dense_topk per chunk of 512 users, train items excluded).

  shape    ML-1M: 6 040 x 3 706, lognormal history lengths (fism_bench.SHAPES), ratings 1 .. 5; towers (64, 32); B = 512 and 4 096
  time     hipEvents around `steps` calls after `warmup` calls, median of `reps` windows; the three step forms alternate window by
           window.  Per-kernel times come from a separate window with the library's launch timing on.
  floor    of the two fused first-layer launches of a step (k_dmf_cut_fan_adam, user and item tower): W1, m, v of both towers read and
           written once, 3 * 2 * (U + I) * H1 * 4 bytes, plus both walked CSRs, nnz * 8 bytes each and their row pointers.  Quoted as
           bytes / time and as a share of the published HBM rate of 8 TB/s (the floor bounds it: no operation count comes near).
Recorded, not gated.  One JSON line on stdout, appended to <out>/dmf_bench.jsonl; the table goes to <out>/dmf_bench.md.

Usage:  python scripts/dmf_bench.py [--steps 20] [--warmup 5] [--reps 5] [--out profiles]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from elliot_amd import ops  # noqa: E402
from elliot_amd.recommender.neural.DMF.deep_matrix_factorization_model import initial_weights as dmf_weights  # noqa: E402
from elliot_amd.recommender.neural.NAIS.nais_model import initial_weights as nais_weights  # noqa: E402
from elliot_amd.synthetic import zipf_csr_device  # noqa: E402
from fism_bench import SHAPES  # noqa: E402
from vbpr_bench import kernel_table, stats, window_ms  # noqa: E402

LR, F, WS, MLP, HBM, CHUNK = 0.001, 64, 32, (64, 32), 8.0e12, 512


def run_batch(ctx, B, steps, warmup, reps):
    s, dev = SHAPES["ml1m_f100"], ctx.device
    U, I = s["U"], s["I"]
    ip, ix = zipf_csr_device(U, I, dev, mean_log=s["mean_log"], sigma_log=1.0, dmin=5, dmax=s["dmax"], seed=5)
    pos, hist = ops.DeviceCSR.from_tensors(ip, ix, I), (ip.cpu().numpy(), ix.cpu().numpy())
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    values = torch.randint(1, 6, (int(ix.numel()),), generator=g, device=dev).float().cpu().numpy()
    dm = ops.DmfDeviceState(ctx, dmf_weights(7, U, I, MLP, MLP), (*hist, values), similarity="cosine", cosine_axis="reference", max_rating=5.0)
    w = {k: v * 50 for k, v in nais_weights(7, U, I, F, WS).items()}
    na = ops.NaisDeviceState(ctx, w, hist)
    fi = ops.FismDeviceState(ctx, w["Gi"], w["Gj"], w["Bu"], w["Bi"], hist)
    batches = []
    for k in range(8):
        u, i, coin = ops.pointwise_sample_ratio(ctx, pos, B, 1, seed=42, first_sample=k * B)
        batches.append((u, i, coin * torch.randint(1, 6, (B,), generator=g, device=dev).float()))
    k = [0]

    def batch():
        k[0] += 1
        return batches[k[0] % len(batches)]

    forms = {"dmf": lambda: dm.train_step(*batch(), LR), "fism": lambda: fi.train_step(*batch(), LR), "nais": lambda: na.train_step(*batch(), LR)}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    win = {n: [] for n in forms}
    for _ in range(reps):
        for n, fn in forms.items():
            win[n].append(window_ms(fn, steps))
    assert all(torch.isfinite(x.loss).all() for x in (dm, fi, na))
    kern = kernel_table(ctx, forms["dmf"], steps)
    floor = 3 * 2 * (U + I) * MLP[0] * 4 + 2 * dm.nnz * 8 + (U + I + 2) * 8
    fan = kern.get("k_dmf_cut_fan_adam")
    out = {"U": U, "I": I, "B": B, "towers": list(MLP), "nnz": dm.nnz, "steps_ms": {n: stats(v) for n, v in win.items()}, "kernels_dmf_ms": kern,
           "fan_adam": {"floor_bytes": floor, "ms": fan, "GB_per_s": None if not fan else floor / fan / 1e6,
                        "share_of_hbm_rate": None if not fan else floor / (fan * 1e-3) / HBM}}

    def evaluation():                                               # the variables changed: towers again, then every chunk
        dm.touch()
        for a in range(0, U, CHUNK):
            dm.recommend(a, min(a + CHUNK, U), 10, excl=pos)

    evaluation()
    out["evaluation"] = stats([window_ms(evaluation, 1) for _ in range(reps)])
    out["kernels_evaluation_ms"] = kernel_table(ctx, evaluation, 1)
    return out


def markdown(res):
    lines = ["# DMF step, fused first-layer Adam and evaluation on one MI355X (scripts/dmf_bench.py)", "",
             f"arch {res['arch']}; ML-1M shape 6 040 x 3 706, towers (64, 32), cosine / reference; {res['steps']} calls per window after "
             f"{res['warmup']} warm-up calls, median of {res['reps']} windows (min .. max beside it); the three step forms alternate window by "
             "window, same process, same samples; FISM and NAIS at F = 64.  The floor of the two `k_dmf_cut_fan_adam` launches of a step: "
             "W1, m, v of both towers read and written once plus both walked CSRs; its share is against the published 8 TB/s of HBM (a "
             "bandwidth bound).  Recorded, not gated.", "",
             "| B | DMF step ms | FISM step ms | NAIS step ms | fan-out + Adam ms per step | floor MB | GB/s | share of 8 TB/s | full evaluation ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    t = lambda x: f"{x['ms']:.3f} ({x['min_ms']:.3f} .. {x['max_ms']:.3f})"                   # noqa: E731
    for B, r in res["batches"].items():
        f = r["fan_adam"]
        rate = (f"not measured | {f['floor_bytes'] / 1e6:.2f} | not measured | not measured" if not f["ms"] else
                f"{f['ms']:.4f} | {f['floor_bytes'] / 1e6:.2f} | {f['GB_per_s']:.0f} | {f['share_of_hbm_rate']:.3f}")
        lines.append(f"| {B} | {t(r['steps_ms']['dmf'])} | {t(r['steps_ms']['fism'])} | {t(r['steps_ms']['nais'])} | {rate} | {t(r['evaluation'])} |")
    for B, r in res["batches"].items():
        for title, key in ((f"B = {B}: per-kernel ms per DMF step", "kernels_dmf_ms"), (f"B = {B}: per-kernel ms per evaluation", "kernels_evaluation_ms")):
            lines += ["", f"## {title} (launch timing on; events between kernels cost their overlap)", "", "| kernel | ms |", "|---|---|"]
            lines += [f"| {k} | {v:.4f} |" for k, v in sorted(r[key].items())]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="512,4096")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "dmf", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "batches": {b: run_batch(ctx, int(b), args.steps, args.warmup, args.reps) for b in args.batches.split(",")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "dmf_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    with open(os.path.join(args.out, "dmf_bench.md"), "w") as f:
        f.write(markdown(res))


if __name__ == "__main__":
    main()
