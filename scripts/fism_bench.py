"""FISM on one MI355X: a FISM step (el_fism_train_step) beside, in the same process and on the same (u, i) pairs, the point-wise step
it is closest to -- el_pwmf_train_step, EL_PW_MSE with both biases, Adam -- on the same U, I, F, B; the forward and fan-out
instantiations of the cut sum as algorithmic bytes over time; the user image and all users' top-10.

  shapes   ml1m_f10 / ml1m_f100   6 040 x 3 706, B = 512 (histories of about 165 items on average)
           configs1               1 000 000 x 100 000, F = 128, B = 2^20 (BASELINE configs[1])
           synthetic positives (zipf_csr), pairs from the ratio sampler (neg_ratio 1), labels its coin times a rating in 1 .. 5
  time     hipEvents around `steps` calls after `warmup` calls, median of `reps` windows, per call; the two step forms alternate
           window by window.  Per-kernel times come from a separate window with the library's launch timing on (events between
           kernels cost their overlap: the per-kernel sum is larger than the step); a rocprofv3 --kernel-trace --stats run of this
           script with --steps-only gives the same kernels without that cost.
  bytes    forward: sum over the batch's distinct users of n_u rows of F floats + 4 bytes per index; fan-out: the same rows back
           (an R row per (item, batch user) pair) + 4 bytes for EVERY nonzero's user id.
Recorded, not gated.  One JSON line on stdout, appended to <out>/fism_bench.jsonl; the table goes to <out>/fism_bench.md.

Usage:  python scripts/fism_bench.py [--steps 20] [--warmup 5] [--reps 5] [--shapes ml1m_f10,ml1m_f100,configs1] [--out profiles] [--steps-only]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr_device  # noqa: E402
from vbpr_bench import kernel_table, stats, window_ms  # noqa: E402

ML1M = dict(U=6040, I=3706, B=512, mean_log=4.5, dmax=2314)
SHAPES = {"ml1m_f10": dict(ML1M, F=10), "ml1m_f100": dict(ML1M, F=100),
          "configs1": dict(U=1000000, I=100000, F=128, B=1 << 20, mean_log=3.0, dmax=1000)}
LR = 0.001
NOTES = """
## What is timed: the reference's model, ported as written

1. the loss is Keras BinaryCrossentropy called as (y_true = out, y_pred = label), in double (`loss: reference`);
2. the regulariser is a sum over the samples and keeps the padded slots of the history matrix (item 0), `pad_len = L`;
3. scoring (`batch_predict`) sums over the padded slots too: the image is `coef_u (p_u + (L - n_u) Gi[0])`;
4. `neg_ratio` is an integer (1 here): a sample is positive with probability 1 / (neg_ratio + 1);
5. Keras Adam on IndexedSlices: every row of all four variables moves every step.
"""


def run_shape(ctx, name, steps, warmup, reps, steps_only):
    s, dev = SHAPES[name], ctx.device
    U, I, F, B = s["U"], s["I"], s["F"], s["B"]
    ip, ix = zipf_csr_device(U, I, dev, mean_log=s["mean_log"], sigma_log=1.0, dmin=5, dmax=s["dmax"], seed=5)
    pos = ops.DeviceCSR.from_tensors(ip, ix, I)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    small = lambda r, c: (torch.rand((r, c), generator=g, device=dev) * 2 - 1) * 0.05             # noqa: E731
    zu, zi = torch.zeros(U, device=dev), torch.zeros(I, device=dev)
    fi = ops.FismDeviceState(ctx, small(I, F), small(I, F), zu, zi, (ip.cpu().numpy(), ix.cpu().numpy()))
    pw = ops.PwmfDeviceState(ctx, small(U, F), small(I, F), zu.clone(), zi.clone(), kind="mse", optimizer="adam")
    batches = []
    for k in range(8):
        u, i, coin = ops.pointwise_sample_ratio(ctx, pos, B, 1, seed=42, first_sample=k * B)
        batches.append((u, i, coin * torch.randint(1, 6, (B,), generator=g, device=dev).float()))
    k = [0]

    def batch():
        k[0] += 1
        return batches[k[0] % len(batches)]

    def fi_step():
        fi.train_step(*batch(), LR)

    def pw_step():
        pw.train_step(*batch(), LR)

    for _ in range(warmup):
        fi_step(), pw_step()
    wf, wp = [], []
    for _ in range(reps):                                           # alternate: both forms see the same neighbours on the machine
        wf.append(window_ms(fi_step, steps))
        wp.append(window_ms(pw_step, steps))
    lens = (ip[1:] - ip[:-1])
    rows = int(lens[torch.unique(batches[0][0]).long()].sum())
    out = {"U": U, "I": I, "F": F, "B": B, "nnz": fi.nnz, "longest_history": fi.longest, "distinct_users": int(torch.unique(batches[0][0]).numel()),
           "rows_each_way": rows, "fism_step": stats(wf), "pwmf_step": stats(wp)}
    out["fism_over_pwmf"] = out["fism_step"]["ms"] / out["pwmf_step"]["ms"]
    assert torch.isfinite(fi.loss).all() and torch.isfinite(pw.loss).all()
    if steps_only:
        return out
    out["kernels_fism_ms"] = kernel_table(ctx, fi_step, steps)
    out["kernels_pwmf_ms"] = kernel_table(ctx, pw_step, steps)
    fwd_bytes, fan_bytes = rows * (F * 4 + 4), rows * F * 4 + fi.nnz * 4
    for key, kern, nbytes in (("forward", "k_fism_cut_fwd", fwd_bytes), ("fan_out", "k_fism_cut_fan", fan_bytes)):
        ms = out["kernels_fism_ms"].get(kern)
        out[key] = {"bytes": nbytes, "ms": ms, "GB_per_s": None if not ms else nbytes / ms / 1e6}
    out["image_build"] = stats([window_ms(fi.image, steps) for _ in range(reps)])
    P, block = fi.image(), min(U, 65536)

    def lists():
        for off in range(0, U, block):
            fi.recommend(P, off, min(off + block, U), 10, excl=pos)

    lists()
    out["top10_all_users"] = stats([window_ms(lists, 3) for _ in range(reps)])
    return out


def markdown(res):
    lines = ["# FISM step and scoring on one MI355X (scripts/fism_bench.py)", "",
             f"arch {res['arch']}; {res['steps']} calls per window after {res['warmup']} warm-up calls, median of {res['reps']} windows "
             "(min - max in brackets); the two step forms alternate window by window, same process, same (u, i) pairs.", "",
             "| shape | U x I | F | B | nnz, longest history | distinct users, rows each way | FISM step ms | point-wise step ms | ratio | "
             "forward GB/s | fan-out GB/s | image build ms | top-10 all users ms |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def cell(x):
        return f"{x['ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"

    def rate(x):
        return "not measured" if not x or not x["GB_per_s"] else f"{x['GB_per_s']:.0f} ({x['ms']:.4f} ms)"
    for name, r in res["shapes"].items():
        lines.append(f"| {name} | {r['U']} x {r['I']} | {r['F']} | {r['B']} | {r['nnz']}, {r['longest_history']} | {r['distinct_users']}, "
                     f"{r['rows_each_way']} | {cell(r['fism_step'])} | {cell(r['pwmf_step'])} | {r['fism_over_pwmf']:.2f} | {rate(r.get('forward'))} | "
                     f"{rate(r.get('fan_out'))} | {cell(r['image_build']) if 'image_build' in r else ''} | "
                     f"{cell(r['top10_all_users']) if 'top10_all_users' in r else ''} |")
    for name, r in res["shapes"].items():
        if "kernels_fism_ms" not in r:
            continue
        lines += ["", f"## {name}: per-kernel ms per step (launch timing on; events between kernels cost their overlap)", "",
                  "| kernel | FISM step | point-wise step |", "|---|---|---|"]
        for kname in sorted(set(r["kernels_fism_ms"]) | set(r["kernels_pwmf_ms"])):
            a, b = r["kernels_fism_ms"].get(kname), r["kernels_pwmf_ms"].get(kname)
            lines.append(f"| {kname} | {'' if a is None else f'{a:.4f}'} | {'' if b is None else f'{b:.4f}'} |")
    return "\n".join(lines) + "\n" + NOTES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m_f10,ml1m_f100,configs1")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--steps-only", action="store_true", help="time the two steps only (the run to put under rocprofv3)")
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "fism", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "shapes": {s: run_shape(ctx, s, args.steps, args.warmup, args.reps, args.steps_only) for s in args.shapes.split(",")}}
    line = json.dumps(res)
    print(line)
    if args.steps_only:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "fism_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    with open(os.path.join(args.out, "fism_bench.md"), "w") as f:
        f.write(markdown(res))


if __name__ == "__main__":
    main()
