"""AMF on one MI355X: an adversarial step (el_amf_grads with EL_AMF_ADVERSARIAL + el_bprmf_apply) beside, in the same process,
the plain pair el_bprmf_grads + el_bprmf_apply on the same tables and batches; and one FGSM and one 20-round MSAP build.

  shapes   ml1m      6 040 x 3 706, F = 200, B = 512 (the reference's AMF defaults); perturbation batch = 800 000 samples
           configs1  1 000 000 x 100 000, F = 128, B = 2^20 (BASELINE configs[1]); perturbation batch = 2^20 samples
           synthetic positives (zipf_csr), triplets from the Philox sampler
  time     hipEvents around `steps` calls after `warmup` calls, median of `reps` windows, per call; the two step forms alternate
           window by window
  bytes    what the algorithm has to move per step, from the shapes and the batch's distinct rows (rows of 4 F bytes):
             gathers   adversarial: forward 6 B (three theta and three delta rows per triplet), segment pass 8 B (a user
                       occurrence reads i, j and their delta rows, each item occurrence u and its delta row), FGSM pass 4 B
                       plain pair : forward fused into the user segments, 4 B (i, j per user occurrence, u per item occurrence)
             rows      one gradient row written per distinct row (+ one delta row written and the old delta rows cleared)
             optimiser 32 bytes per parameter in both (theta, m, v read and written, the accumulator read and cleared)
Recorded, not gated.  One JSON line on stdout, appended to profiles/amf_bench.jsonl.

Usage:  python scripts/amf_bench.py [--steps 20] [--warmup 5] [--reps 5] [--shapes ml1m,configs1]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr_device  # noqa: E402

SHAPES = {"ml1m": dict(U=6040, I=3706, F=200, B=512, full=800000, mean_log=4.5, dmax=2000),
          "configs1": dict(U=1000000, I=100000, F=128, B=1 << 20, full=1 << 20, mean_log=3.0, dmax=1000)}
L_W, L_B, EPS, L_ADV, LR = 0.1, 0.001, 0.1, 0.001, 0.001            # AMF.py:82-92 defaults


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def stats(w):
    w = sorted(w)
    return {"ms": w[len(w) // 2], "min_ms": w[0], "max_ms": w[-1]}


def run_shape(ctx, name, steps, warmup, reps):
    s, dev = SHAPES[name], ctx.device
    U, I, F, B = s["U"], s["I"], s["F"], s["B"]
    ip, ix = zipf_csr_device(U, I, dev, mean_log=s["mean_log"], sigma_log=1.0, dmin=5, dmax=s["dmax"], seed=5)
    pos = ops.DeviceCSR.from_tensors(ip, ix, I)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    lu, li = (6.0 / (U + F)) ** 0.5, (6.0 / (I + F)) ** 0.5
    st = ops.AmfDeviceState(ctx, (torch.rand((U, F), generator=g, device=dev) * 2 - 1) * lu,
                            (torch.rand((I, F), generator=g, device=dev) * 2 - 1) * li, torch.zeros(I, device=dev))
    batches = [ops.bpr_sample(ctx, pos, B, seed=42, first_sample=k * B) for k in range(8)]
    k = [0]

    def batch():
        k[0] += 1
        return batches[k[0] % len(batches)]

    def adversarial():
        st.train_step(*batch(), LR, L_W, L_B, L_ADV, EPS, True)

    def plain():
        st.base.grads(*batch(), L_W, L_B)
        st.base.apply(LR)

    for _ in range(warmup):
        adversarial(), plain()
    wa, wp = [], []
    for _ in range(reps):                                           # alternate: both forms see the same neighbours on the machine
        wa.append(window_ms(adversarial, steps))
        wp.append(window_ms(plain, steps))
    out = {"U": U, "I": I, "F": F, "B": B, "adversarial_step": stats(wa), "plain_pair": stats(wp)}
    out["apply"] = stats([window_ms(lambda: st.base.apply(LR), steps) for _ in range(reps)])
    assert torch.isfinite(st.loss).all()
    st.pop_loss()
    u, i, j = batches[0]
    rows = int(torch.unique(u).numel() + torch.unique(torch.cat([i, j])).numel())
    row, par = 4 * F, (U + I) * F + I
    out["distinct_rows"] = rows
    out["bytes_adversarial"] = (6 + 8 + 4) * B * row + 3 * rows * row + 32 * par
    out["bytes_plain"] = 4 * B * row + rows * row + 32 * par
    out["bytes_optimiser"] = 32 * par
    out["adversarial_over_plain"] = out["adversarial_step"]["ms"] / out["plain_pair"]["ms"]
    grads_a = out["adversarial_step"]["ms"] - out["apply"]["ms"]
    grads_p = out["plain_pair"]["ms"] - out["apply"]["ms"]
    out["gradient_pass_ms"] = {"adversarial": grads_a, "plain": grads_p, "ratio": grads_a / grads_p if grads_p > 0 else None}
    # the perturbations of evaluate_perturbations: one batch of `full` samples
    fu, fi, fj = ops.bpr_sample(ctx, pos, s["full"], seed=43)
    for _ in range(2):
        st.perturb(fu, fi, fj, L_W, L_B, EPS)
    out["fgsm_full_batch"] = stats([window_ms(lambda: st.perturb(fu, fi, fj, L_W, L_B, EPS), 3) for _ in range(reps)])
    st.perturb(fu, fi, fj, L_W, L_B, EPS, 2.5 * EPS / 20, 20)
    out["msap20_full_batch"] = stats([window_ms(lambda: st.perturb(fu, fi, fj, L_W, L_B, EPS, 2.5 * EPS / 20, 20), 1) for _ in range(reps)])
    out["full_batch"] = s["full"]
    out["bytes_fgsm"] = (3 + 4) * s["full"] * row
    out["bytes_msap20"] = 20 * (6 + 8) * s["full"] * row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,configs1")
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "amf", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "shapes": {s: run_shape(ctx, s, args.steps, args.warmup, args.reps) for s in args.shapes.split(",")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "amf_bench.jsonl"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
