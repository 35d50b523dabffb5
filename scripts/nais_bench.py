"""NAIS on one MI355X: a NAIS step (el_nais_train_step) beside, in the same process and on the same samples, the FISM step
(el_fism_train_step) it is built on; the three pair-walking kernels as pairs, algorithmic bytes and 3 * 2F operations per pair over
time; the top-10 of the first users (512, or 2 000 000 / I where that is fewer) through el_nais_scores + el_dense_topk as (their nnz) * I * 2F
inner-loop steps against the fp32 vector peak.

  shapes   ml1m_f10 / ml1m_f100   6 040 x 3 706, B = 512, Ws = 32 (histories of about 165 items on average)
           configs1               1 000 000 x 100 000, F = 128, B = 2^20 (BASELINE configs[1]; a step walks about 10^8 pairs, so
                                  its windows are at most 3 steps after 1 warm-up step, 3 windows)
  time     hipEvents around `steps` calls after `warmup` calls, median of `reps` windows; the two step forms alternate window by
           window.  Per-kernel times come from a separate window with the library's launch timing on.
  pairs    sample-major walks: sum over the samples of n_u; fan-out: sum over the samples of n_u as well (every pair is met once from
           its item's side).  bytes per pair: forward and backward a Gi row and an A row (3F floats; the backward reads them twice),
           fan-out a Gj row and a Bt row (3F floats); + 4 bytes per index.
  peak     the published fp32 vector peak, 157.3 TFLOP/s = 78.6 T lane-instructions / s (it counts the packed two-wide forms, which
           this source file is built without: the share quoted is against the card, not against the build); a step of the
           scoring loop is 3 instructions (add, max, fma), so 26.2 T steps / s is the bound quoted.
Recorded, not gated.  One JSON line on stdout, appended to <out>/nais_bench.jsonl; the table goes to <out>/nais_bench.md.

Usage:  python scripts/nais_bench.py [--steps 20] [--warmup 5] [--reps 5] [--shapes ml1m_f10,ml1m_f100,configs1] [--out profiles]
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
from elliot_amd.recommender.neural.NAIS.nais_model import initial_weights  # noqa: E402
from elliot_amd.synthetic import zipf_csr_device  # noqa: E402
from fism_bench import SHAPES  # noqa: E402
from vbpr_bench import kernel_table, stats, window_ms  # noqa: E402

LR, WS, PEAK_STEPS = 0.001, 32, 157.3e12 / 2 / 3


def run_shape(ctx, name, steps, warmup, reps):
    s, dev = SHAPES[name], ctx.device
    U, I, F, B = s["U"], s["I"], s["F"], s["B"]
    ip, ix = zipf_csr_device(U, I, dev, mean_log=s["mean_log"], sigma_log=1.0, dmin=5, dmax=s["dmax"], seed=5)
    pos, hist = ops.DeviceCSR.from_tensors(ip, ix, I), (ip.cpu().numpy(), ix.cpu().numpy())
    w = {k: v * 50 for k, v in initial_weights(7, U, I, F, WS).items()}                   # (+-0.05 as fism_bench.py draws its tables)
    na = ops.NaisDeviceState(ctx, w, hist)
    fi = ops.FismDeviceState(ctx, w["Gi"], w["Gj"], w["Bu"], w["Bi"], hist)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    batches = []
    for k in range(8):
        u, i, coin = ops.pointwise_sample_ratio(ctx, pos, B, 1, seed=42, first_sample=k * B)
        batches.append((u, i, coin * torch.randint(1, 6, (B,), generator=g, device=dev).float()))
    k = [0]

    def batch():
        k[0] += 1
        return batches[k[0] % len(batches)]

    na_step, fi_step = (lambda: na.train_step(*batch(), LR)), (lambda: fi.train_step(*batch(), LR))
    for _ in range(warmup):
        na_step(), fi_step()
    wn, wf = [], []
    for _ in range(reps):
        wn.append(window_ms(na_step, steps))
        wf.append(window_ms(fi_step, steps))
    assert torch.isfinite(na.loss).all() and torch.isfinite(fi.loss).all()
    lens = (ip[1:] - ip[:-1])
    pairs = float(np.mean([int(lens[b[0].long()].sum()) for b in batches]))
    out = {"U": U, "I": I, "F": F, "B": B, "Ws": WS, "nnz": na.nnz, "longest_history": na.longest, "pairs_per_step": pairs,
           "nais_step": stats(wn), "fism_step": stats(wf), "kernels_nais_ms": kernel_table(ctx, na_step, steps)}
    out["nais_over_fism"] = out["nais_step"]["ms"] / out["fism_step"]["ms"]
    for kern, reads in (("k_nais_fwd", 1), ("k_nais_bwd", 2), ("k_nais_fan", 1)):
        ms = out["kernels_nais_ms"].get(kern)
        nbytes = pairs * (reads * 3 * F * 4 + 4)
        out[kern] = {"pairs": pairs, "bytes": nbytes, "ms": ms, "GB_per_s": None if not ms else nbytes / ms / 1e6,
                     "Gop_per_s": None if not ms else pairs * 3 * 2 * F / ms / 1e6}
    block = min(512, max(8, 2000000 // I))

    def lists():                                                    # (ONE block of users: all users of the F = 100 shape take minutes)
        na.recommend(0, min(block, U), 10, excl=pos)

    lists()
    out["score_users"] = min(block, U)
    out["top10_block"] = stats([window_ms(lists, 1) for _ in range(reps)])
    out["score_steps"] = float(ip[min(block, U)]) * I * 2 * F
    out["score_kernel_ms"] = kernel_table(ctx, lists, 1).get("k_nais_scores")
    if out["score_kernel_ms"]:
        out["score_fraction_of_vector_peak"] = out["score_steps"] / (out["score_kernel_ms"] * 1e-3) / PEAK_STEPS
    return out


def markdown(res):
    lines = ["# NAIS step and scoring on one MI355X (scripts/nais_bench.py)", "",
             f"arch {res['arch']}; {res['steps']} calls per window after {res['warmup']} warm-up calls, median of {res['reps']} windows; the two "
             "step forms alternate window by window, same process, same samples.", "",
             "| shape | F | B | pairs per step | NAIS step ms | FISM step ms | ratio | fwd ms, GB/s, Gop/s | bwd ms, GB/s, Gop/s | fan-out ms, GB/s, Gop/s | "
             "users scored, their top-10 ms | k_nais_scores ms, share of the fp32 vector peak |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rate = lambda x: "not measured" if not x["ms"] else f"{x['ms']:.3f}, {x['GB_per_s']:.0f}, {x['Gop_per_s']:.0f}"        # noqa: E731
    for name, r in res["shapes"].items():
        sk = r.get("score_kernel_ms")
        sc = "not measured" if not sk else f"{sk:.1f}, {r['score_fraction_of_vector_peak']:.3f}"
        lines.append(f"| {name} | {r['F']} | {r['B']} | {r['pairs_per_step']:.0f} | {r['nais_step']['ms']:.3f} | {r['fism_step']['ms']:.3f} | "
                     f"{r['nais_over_fism']:.1f} | {rate(r['k_nais_fwd'])} | {rate(r['k_nais_bwd'])} | {rate(r['k_nais_fan'])} | "
                     f"{r['score_users']}, {r['top10_block']['ms']:.1f} | {sc} |")
    for name, r in res["shapes"].items():
        lines += ["", f"## {name}: per-kernel ms per NAIS step (launch timing on; events between kernels cost their overlap)", "", "| kernel | ms |", "|---|---|"]
        lines += [f"| {k} | {v:.4f} |" for k, v in sorted(r["kernels_nais_ms"].items())]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m_f10,ml1m_f100")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "nais", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "shapes": {s: run_shape(ctx, s, *((min(args.steps, 3), min(args.warmup, 1), min(args.reps, 3)) if s == "configs1" else
                                             (args.steps, args.warmup, args.reps))) for s in args.shapes.split(",")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "nais_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    with open(os.path.join(args.out, "nais_bench.md"), "w") as f:
        f.write(markdown(res))


if __name__ == "__main__":
    main()
