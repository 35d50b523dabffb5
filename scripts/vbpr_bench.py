"""VBPR on one MI355X: a VBPR step (el_vbpr_grads + el_vbpr_apply) beside, in the same process and on the same triplets, the plain
pair el_bprmf_grads + el_bprmf_apply on the same Gu / Gi / Bi; and the scoring image + all users' top-10 beside el_score_topk on
the plain tables.

  shapes   ml1m      6 040 x 3 706, F = 100, Fd = 20, D = 2048, B = 512 (the reference's VBPR defaults) and B = 4096 on the same
                     catalogue: two batch sizes show whether feature traffic follows the batch's DISTINCT items
           configs1  1 000 000 x 100 000, F = 128, Fd = 20, D = 2048, B = 2^20 (BASELINE configs[1])
           synthetic positives (zipf_csr), triplets from the Philox sampler, random non-negative features
  time     hipEvents around `steps` calls after `warmup` calls, median of `reps` windows, per call; the two step forms alternate
           window by window.  Per-kernel times come from a separate window with the library's launch timing on (events between
           kernels cost their overlap: the per-kernel sum is larger than the step).
  bytes    what the algorithm has to move per step, from the shapes and n = the batch's distinct items:
             features  n D 4 bytes per read of Feat_rows: two reads (forward and backward product), plus one read and one write
                       for the gather when n < I (with n = I the products read the matrix in place)
             rows      forward 3 B rows of (F + Fd) floats, segment pass 4 B rows (a user occurrence reads i and j, each item
                       occurrence u), one gradient row written per distinct row, n rows of Fd + 1 floats for P and for [A | a]
             dense     E | Bp: read forward, gradient written, regulariser read + write, optimiser 28 bytes per element
             optimiser 32 bytes per parameter of Gu, Gi, Bi, Tu (theta, m, v read and written, the accumulator read and cleared)
Recorded, not gated.  One JSON line on stdout, appended to <out>/vbpr_bench.jsonl; the table goes to <out>/vbpr_bench.md.

Usage:  python scripts/vbpr_bench.py [--steps 20] [--warmup 5] [--reps 5] [--shapes ml1m,ml1m_b4096,configs1] [--out profiles]
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

SHAPES = {"ml1m": dict(U=6040, I=3706, F=100, Fd=20, D=2048, B=512, mean_log=4.5, dmax=2000),
          "ml1m_b4096": dict(U=6040, I=3706, F=100, Fd=20, D=2048, B=4096, mean_log=4.5, dmax=2000),
          "configs1": dict(U=1000000, I=100000, F=128, Fd=20, D=2048, B=1 << 20, mean_log=3.0, dmax=1000)}
L_W, L_B, L_E, LR = 0.000025, 0.0, 0.002, 0.0005                      # VBPR.py:60-69 defaults


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


def kernel_table(ctx, fn, steps):
    """{kernel: ms per call of fn} from the library's own launch timing."""
    ctx.timing(True)
    try:
        ctx.timing_report()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        rep = ctx.timing_report()
    finally:
        ctx.timing(False)
    return {k: ms / steps for k, (_, ms) in sorted(rep.items())}


def run_shape(ctx, name, steps, warmup, reps):
    s, dev = SHAPES[name], ctx.device
    U, I, F, Fd, D, B = s["U"], s["I"], s["F"], s["Fd"], s["D"], s["B"]
    ip, ix = zipf_csr_device(U, I, dev, mean_log=s["mean_log"], sigma_log=1.0, dmin=5, dmax=s["dmax"], seed=5)
    pos = ops.DeviceCSR.from_tensors(ip, ix, I)
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def glorot(rows, cols):
        return (torch.rand((rows, cols), generator=g, device=dev) * 2 - 1) * (6.0 / (rows + cols)) ** 0.5
    feat = torch.clamp(torch.randn((I, D), generator=g, device=dev), min=0).contiguous()
    st = ops.VbprDeviceState(ctx, glorot(U, F), glorot(I, F), torch.zeros(I, device=dev), glorot(U, Fd), glorot(D, Fd), glorot(D, 1), feat)
    batches = [ops.bpr_sample(ctx, pos, B, seed=42, first_sample=k * B) for k in range(8)]
    k = [0]

    def batch():
        k[0] += 1
        return batches[k[0] % len(batches)]

    def vbpr():
        st.train_step(*batch(), LR, L_W, L_B, L_E)

    def plain():
        st.base.grads(*batch(), L_W, L_B)
        st.base.apply(LR)

    for _ in range(warmup):
        vbpr(), plain()
    wv, wp = [], []
    for _ in range(reps):                                           # alternate: both forms see the same neighbours on the machine
        wv.append(window_ms(vbpr, steps))
        wp.append(window_ms(plain, steps))
    out = {"U": U, "I": I, "F": F, "Fd": Fd, "D": D, "B": B, "vbpr_step": stats(wv), "plain_pair": stats(wp)}
    out["vbpr_over_plain"] = out["vbpr_step"]["ms"] / out["plain_pair"]["ms"]
    # the gradient half alone (its stores overwrite: it can run back to back; the accumulators are cleared behind the windows)
    out["vbpr_grads"] = stats([window_ms(lambda: st.grads(*batch(), L_W, L_B, L_E), steps) for _ in range(reps)])
    for t in (st.gTu, st.gEB, st.base.gGu, st.base.item_grad_flat):
        t.zero_()
    assert torch.isfinite(st.loss).all()
    st.pop_loss()
    out["kernels_vbpr_ms"] = kernel_table(ctx, vbpr, steps)
    out["kernels_plain_ms"] = kernel_table(ctx, plain, steps)
    ksum = sum(out["kernels_vbpr_ms"].values())
    prod = sum(v for n, v in out["kernels_vbpr_ms"].items() if n.startswith("k_gemm"))
    out["products_ms"], out["products_share_of_kernel_sum"] = prod, prod / ksum if ksum else None
    u, i, j = batches[0]
    n = int(torch.unique(torch.cat([i, j])).numel())
    nu = int(torch.unique(u).numel())
    st.grads(u, i, j, L_W, L_B, L_E)
    assert st.last_distinct_items == n
    st.apply(LR)
    W, N = F + Fd, Fd + 1
    out["distinct_items"], out["distinct_users"] = n, nu
    out["bytes_features"] = n * D * 4 * (2 if n == I else 4)
    out["bytes_rows"] = (3 + 4) * B * W * 4 + (nu + n) * W * 4 + 2 * 2 * n * N * 4
    out["bytes_dense"] = D * N * 4 * (1 + 1 + 2) + 28 * D * N
    out["bytes_optimiser"] = 32 * ((U + I) * F + I + U * Fd)
    out["bytes_vbpr"] = out["bytes_features"] + out["bytes_rows"] + out["bytes_dense"] + out["bytes_optimiser"]
    out["bytes_plain"] = 4 * B * F * 4 + (nu + n) * F * 4 + 32 * ((U + I) * F + I)
    out["flops_products"] = 2 * 2 * n * D * N
    # scoring: the image of all items + every user's top-10, beside the top-10 on the plain tables
    out["image_build"] = stats([window_ms(st.image, steps) for _ in range(reps)])
    P, Q, bq = st.image()
    block = min(U, 65536)

    def lists(Pu, Qi, b):
        for off in range(0, U, block):
            ops.score_topk(ctx, Pu, Qi, b, off, min(off + block, U), 10, excl=pos)

    lists(P, Q, bq), lists(st.base.Gu, st.base.Gi, st.base.Bi)
    tv, tp = [], []
    for _ in range(reps):
        tv.append(window_ms(lambda: lists(P, Q, bq), 3))
        tp.append(window_ms(lambda: lists(st.base.Gu, st.base.Gi, st.base.Bi), 3))
    out["top10_all_users_vbpr"], out["top10_all_users_plain"] = stats(tv), stats(tp)
    return out


def markdown(res):
    lines = ["# VBPR step and scoring on one MI355X (scripts/vbpr_bench.py)", "",
             f"arch {res['arch']}; {res['steps']} calls per window after {res['warmup']} warm-up calls, median of {res['reps']} windows "
             "(min - max in brackets); the two step forms alternate window by window, same process, same triplets.", "",
             "| shape | U x I | F + Fd, D | B | distinct items | VBPR step ms | plain BPR pair ms | ratio | VBPR grads ms | products ms "
             "(share of kernel sum) | feature bytes / step | image build ms | top-10 all users: VBPR / plain ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def cell(x):
        return f"{x['ms']:.3f} ({x['min_ms']:.3f} - {x['max_ms']:.3f})"
    for name, r in res["shapes"].items():
        lines.append(f"| {name} | {r['U']} x {r['I']} | {r['F']} + {r['Fd']}, {r['D']} | {r['B']} | {r['distinct_items']} | "
                     f"{cell(r['vbpr_step'])} | {cell(r['plain_pair'])} | {r['vbpr_over_plain']:.2f} | {cell(r['vbpr_grads'])} | "
                     f"{r['products_ms']:.3f} ({100 * r['products_share_of_kernel_sum']:.0f} %) | {r['bytes_features'] / 1e6:.1f} MB | "
                     f"{cell(r['image_build'])} | {cell(r['top10_all_users_vbpr'])} / {cell(r['top10_all_users_plain'])} |")
    for name, r in res["shapes"].items():
        lines += ["", f"## {name}: per-kernel ms per step (launch timing on; events between kernels cost their overlap)", "",
                  "| kernel | VBPR step | plain pair |", "|---|---|---|"]
        for kname in sorted(set(r["kernels_vbpr_ms"]) | set(r["kernels_plain_ms"])):
            a, b = r["kernels_vbpr_ms"].get(kname), r["kernels_plain_ms"].get(kname)
            lines.append(f"| {kname} | {'' if a is None else f'{a:.4f}'} | {'' if b is None else f'{b:.4f}'} |")
        lines += ["", f"algorithmic bytes per step: VBPR {r['bytes_vbpr'] / 1e6:.1f} MB (features {r['bytes_features'] / 1e6:.1f}, rows "
                  f"{r['bytes_rows'] / 1e6:.1f}, E | Bp {r['bytes_dense'] / 1e6:.2f}, optimiser {r['bytes_optimiser'] / 1e6:.1f}); plain pair "
                  f"{r['bytes_plain'] / 1e6:.1f} MB; the two products: {r['flops_products'] / 1e9:.2f} GFLOP"]
    a, b = res["shapes"].get("ml1m"), res["shapes"].get("ml1m_b4096")
    if a and b:                                                      # two batch sizes over one catalogue: does feature work follow n?
        def feature_ms(r):
            return sum(v for n, v in r["kernels_vbpr_ms"].items() if n.startswith("k_gemm") or n == "k_vbpr_gather")
        lines += ["", "## Feature traffic against the batch's distinct items (ML-1M catalogue, B = 512 and B = 4096)", "",
                  f"B x {b['B'] / a['B']:.0f}; distinct items {a['distinct_items']} -> {b['distinct_items']} "
                  f"(x {b['distinct_items'] / a['distinct_items']:.2f}); algorithmic feature bytes {a['bytes_features'] / 1e6:.1f} -> "
                  f"{b['bytes_features'] / 1e6:.1f} MB (x {b['bytes_features'] / a['bytes_features']:.2f}); gather + the two products "
                  f"{feature_ms(a):.4f} -> {feature_ms(b):.4f} ms (x {feature_ms(b) / feature_ms(a):.2f})"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,ml1m_b4096,configs1")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "vbpr", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "shapes": {s: run_shape(ctx, s, args.steps, args.warmup, args.reps) for s in args.shapes.split(",")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "vbpr_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    with open(os.path.join(args.out, "vbpr_bench.md"), "w") as f:
        f.write(markdown(res))


if __name__ == "__main__":
    main()
