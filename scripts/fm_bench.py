"""FM on one MI355X: an FM step (el_fm_train_step) beside, in the same process and on the same (u, i) pairs, the point-wise step it
is closest to -- el_pwmf_train_step, EL_PW_MSE with both biases, Adam -- on the same U, I, F, B; the fan-out kernels alone on a
catalogue where one feature sits on half the items; and the item image + all users' top-10 beside el_score_topk on plain tables.

  shapes   ml1m_f10 / ml1m_f64   6 040 x 3 706, B = 512, 10 000 features, about 20 per item
           ml1m_f64_half         the same with feature 0 on every other item (the long-list route of k_fm_feat)
           configs1              1 000 000 x 100 000, F = 128, B = 2^20, 5 000 features, about 10.5 per item (BASELINE configs[1])
           the assumed attribute statistics and the generator of scripts/attr_bench.py; synthetic positives (zipf_csr), pairs from
           the Philox point-wise sampler, labels its coin times a rating in 1 .. 5
  time     hipEvents around `steps` calls after `warmup` calls, median of `reps` windows, per call; the two step forms alternate
           window by window.  Per-kernel times come from a separate window with the library's launch timing on (events between
           kernels cost their overlap: the per-kernel sum is larger than the step).
Recorded, not gated.  One JSON line on stdout, appended to <out>/fm_bench.jsonl; the table goes to <out>/fm_bench.md.

Usage:  python scripts/fm_bench.py [--steps 20] [--warmup 5] [--reps 5] [--shapes ml1m_f10,ml1m_f64,ml1m_f64_half,configs1] [--out profiles]
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

from attr_bench import item_features  # noqa: E402
from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr_device  # noqa: E402
from vbpr_bench import kernel_table, stats, window_ms  # noqa: E402

ML1M = dict(U=6040, I=3706, B=512, nF=10000, per_item=20, mean_log=4.5, dmax=2000)
SHAPES = {"ml1m_f10": dict(ML1M, F=10), "ml1m_f64": dict(ML1M, F=64), "ml1m_f64_half": dict(ML1M, F=64, half=True),
          "configs1": dict(U=1000000, I=100000, F=128, B=1 << 20, nF=5000, per_item=10, mean_log=3.0, dmax=1000)}
LR = 0.001


def run_shape(ctx, name, steps, warmup, reps):
    s, dev = SHAPES[name], ctx.device
    U, I, F, B, nF = s["U"], s["I"], s["F"], s["B"], s["nF"]
    ip, ix = zipf_csr_device(U, I, dev, mean_log=s["mean_log"], sigma_log=1.0, dmin=5, dmax=s["dmax"], seed=5)
    pos = ops.DeviceCSR.from_tensors(ip, ix, I)
    A, _ = item_features(I, nF, s["per_item"], seed=11)
    feats = [A.indices[A.indptr[i]:A.indptr[i + 1]].tolist() + ([0] if s.get("half") and i % 2 else []) for i in range(I)]
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def glorot(rows, cols):
        return (torch.rand((rows, cols), generator=g, device=dev) * 2 - 1) * (6.0 / (rows + cols)) ** 0.5
    fm = ops.FmDeviceState(ctx, U, I, glorot(U + I + nF, F), item_features=feats, n_features=nF)
    pw = ops.PwmfDeviceState(ctx, glorot(U, F), glorot(I, F), torch.zeros(U, device=dev), torch.zeros(I, device=dev), kind="mse", optimizer="adam")
    batches = []
    for k in range(8):
        u, i, coin = ops.pointwise_sample(ctx, pos, B, seed=42, first_sample=k * B)
        batches.append((u, i, coin * torch.randint(1, 6, (B,), generator=g, device=dev).float()))
    k = [0]

    def batch():
        k[0] += 1
        return batches[k[0] % len(batches)]

    def fm_step():
        fm.train_step(*batch(), LR)

    def pw_step():
        pw.train_step(*batch(), LR)

    for _ in range(warmup):
        fm_step(), pw_step()
    wf, wp = [], []
    for _ in range(reps):                                           # alternate: both forms see the same neighbours on the machine
        wf.append(window_ms(fm_step, steps))
        wp.append(window_ms(pw_step, steps))
    nnz = int(fm.index[0][-1])
    out = {"U": U, "I": I, "F": F, "B": B, "nF": nF, "nnz_attributes": nnz, "longest_feature_list": int(np.diff(fm.index[2]).max()),
           "distinct_items": int(torch.unique(batches[0][1]).numel()), "fm_step": stats(wf), "pwmf_step": stats(wp)}
    out["fm_over_pwmf"] = out["fm_step"]["ms"] / out["pwmf_step"]["ms"]
    assert torch.isfinite(fm.loss).all() and torch.isfinite(pw.loss).all()
    out["kernels_fm_ms"] = kernel_table(ctx, fm_step, steps)
    out["kernels_pwmf_ms"] = kernel_table(ctx, pw_step, steps)
    # scoring: the image of all items + every user's top-10, beside the top-10 on the plain tables with both biases
    out["image_build"] = stats([window_ms(fm.image, steps) for _ in range(reps)])
    Q, bq = fm.image()
    block = min(U, 65536)

    def lists_fm():
        for off in range(0, U, block):
            fm.recommend(Q, bq, off, min(off + block, U), 10, excl=pos)

    def lists_pw():
        for off in range(0, U, block):
            pw.recommend(off, min(off + block, U), 10, excl=pos)

    lists_fm(), lists_pw()
    tf, tp = [], []
    for _ in range(reps):
        tf.append(window_ms(lists_fm, 3))
        tp.append(window_ms(lists_pw, 3))
    out["top10_all_users_fm"], out["top10_all_users_pwmf"] = stats(tf), stats(tp)
    return out


def markdown(res):
    lines = ["# FM step and scoring on one MI355X (scripts/fm_bench.py)", "",
             f"arch {res['arch']}; {res['steps']} calls per window after {res['warmup']} warm-up calls, median of {res['reps']} windows "
             "(min - max in brackets); the two step forms alternate window by window, same process, same (u, i) pairs.", "",
             "| shape | U x I | F | B | features, nnz, longest list | distinct items | FM step ms | point-wise step ms | ratio | image build ms | "
             "top-10 all users: FM / point-wise ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]

    def cell(x):
        return f"{x['ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"
    for name, r in res["shapes"].items():
        lines.append(f"| {name} | {r['U']} x {r['I']} | {r['F']} | {r['B']} | {r['nF']}, {r['nnz_attributes']}, {r['longest_feature_list']} | "
                     f"{r['distinct_items']} | {cell(r['fm_step'])} | {cell(r['pwmf_step'])} | {r['fm_over_pwmf']:.2f} | {cell(r['image_build'])} | "
                     f"{cell(r['top10_all_users_fm'])} / {cell(r['top10_all_users_pwmf'])} |")
    for name, r in res["shapes"].items():
        lines += ["", f"## {name}: per-kernel ms per step (launch timing on; events between kernels cost their overlap)", "",
                  "| kernel | FM step | point-wise step |", "|---|---|---|"]
        for kname in sorted(set(r["kernels_fm_ms"]) | set(r["kernels_pwmf_ms"])):
            a, b = r["kernels_fm_ms"].get(kname), r["kernels_pwmf_ms"].get(kname)
            lines.append(f"| {kname} | {'' if a is None else f'{a:.4f}'} | {'' if b is None else f'{b:.4f}'} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m_f10,ml1m_f64,ml1m_f64_half,configs1")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "fm", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "shapes": {s: run_shape(ctx, s, args.steps, args.warmup, args.reps) for s in args.shapes.split(",")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "fm_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    with open(os.path.join(args.out, "fm_bench.md"), "w") as f:
        f.write(markdown(res))


if __name__ == "__main__":
    main()
