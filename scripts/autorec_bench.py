"""UserAutoRec / ItemAutoRec on one MI355X: one train step on the batch's nonzeros (el_autorec_train_step) beside the three dense
B x N x H products the reference's route multiplies around the 99 %-zero batch block, and beside the dense Adam pass alone.

  shapes     user-ml1m   6 040 rows x 3 706 columns        item-ml1m   3 706 rows x 6 040 columns (the transpose of the same matrix)
             user-ml20m  138 493 rows x 26 744 columns     -- synthetic (zipf_csr), H = 500, B = 512
  step       el_autorec_train_step on successive batches of a fixed permutation: hipEvents around `steps` calls after `warmup` calls,
             median of `reps` windows, per step
  grads      el_autorec_grads alone, the same way (step - grads ~ the Adam pass inside the step)
  adam       el_autorec_apply alone, the same way; its bytes (theta, m, v read and written, g read: 28 bytes per parameter) per second
  dense      three el_gemm_f32 products of 2 B N H flops each in the same run: [B,N] x [N,H] (encoder), [B,H] x [H,N] (decoder),
             [B,N] x [N,H] (the hidden layer's gradient) -- a LOWER bound of the reference's route (its weight gradients are two more)
  entries    the batch's mean number of entries: the decoder work that matters is 4 H flops per entry forward, 4 H backward
Recorded, not gated.  One JSON line on stdout, appended to profiles/autorec_bench.jsonl.

Usage:  python scripts/autorec_bench.py [--steps 50] [--warmup 10] [--reps 5] [--shapes user-ml1m,item-ml1m,user-ml20m]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from elliot_amd import ops  # noqa: E402
from elliot_amd.synthetic import zipf_csr, zipf_csr_device  # noqa: E402

H, B = 500, 512


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(fn, steps, warmup, reps):
    for _ in range(warmup):
        fn()
    w = sorted(window_ms(fn, steps) for _ in range(reps))
    return {"ms": w[reps // 2], "min_ms": w[0], "max_ms": w[-1]}


def matrix(ctx, shape):
    if shape == "user-ml20m":
        ip, ix = zipf_csr_device(138493, 26744, ctx.device, mean_log=4.5, sigma_log=1.0, dmin=20, dmax=3000, seed=5)
        return ops.DeviceCSR.from_tensors(ip, ix, 26744), "linear"
    ip, ix = zipf_csr(6040, 3706, mean_log=4.5, sigma_log=1.0, dmin=20, dmax=2000, seed=5)
    m = sp.csr_matrix((np.ones(len(ix), np.float32), ix, ip), shape=(6040, 3706))
    if shape == "item-ml1m":
        return ops.DeviceCSR.from_scipy(m.T, ctx.device), "sigmoid"
    return ops.DeviceCSR.from_scipy(m, ctx.device), "linear"


def run_shape(ctx, shape, steps, warmup, reps):
    dev = ctx.device
    csr, head = matrix(ctx, shape)
    R, N = int(csr.n_rows), int(csr.n_cols)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    gn = lambda a, b: torch.randn((a, b), generator=g, device=dev) * (2.0 / (a + b)) ** 0.5       # GlorotNormal scale
    lens = csr.indptr[1:] - csr.indptr[:-1]
    nnz_max = int(torch.topk(lens, min(B, R)).values.sum().item())
    st = ops.AutoRecDeviceState(ctx, {"W1": gn(N, H), "b1": torch.ones(H, device=dev), "W2": gn(H, N), "b2": torch.ones(N, device=dev)},
                                None if head == "linear" else head, max_batch=B, nnz_max=nnz_max)
    perm = torch.randperm(R, device=dev, generator=g).to(torch.int32)
    nb = R // B
    it = [0]

    def batch():
        b = it[0] % nb
        it[0] += 1
        return perm[b * B:(b + 1) * B]

    out = {"rows": R, "N": N, "H": H, "B": B, "head": head, "nnz": int(csr.nnz),
           "entries_per_batch": float(lens[perm[:nb * B].long()].sum().item()) / nb}
    out["step"] = measure(lambda: st.train_step(csr, batch(), 0.0001), steps, warmup, reps)
    loss = st.pop_loss()
    assert np.isfinite(loss), loss
    out["grads"] = measure(lambda: st.grads(csr, batch()), steps, warmup, reps)
    st.pop_loss()
    out["adam"] = measure(lambda: st.apply(0.0001), steps, warmup, reps)
    n_par = 2 * N * H + H + N
    out["adam"]["bytes"] = 28 * n_par
    out["adam"]["TB_per_s"] = 28 * n_par / (out["adam"]["ms"] * 1e-3) / 1e12
    # the dense route's products on a [B, N] block (its content does not change their time)
    X = torch.zeros((B, N), device=dev)
    hbuf, rbuf, dbuf = torch.empty((B, H), device=dev), torch.empty((B, N), device=dev), torch.empty((B, H), device=dev)

    def dense():
        ops.gemm(ctx, X, st.w[0], out=hbuf, bias=st.w[1], act="sigmoid")                   # encoder: [B,N] x [N,H]
        ops.gemm(ctx, hbuf, st.w[2], transB=True, out=rbuf, bias=st.w[3])                   # decoder: [B,H] x [H,N]
        ops.gemm(ctx, rbuf, st.w[2], out=dbuf)                                              # dh = dpre W2^T: [B,N] x [N,H]
    out["dense3"] = measure(dense, steps, warmup, reps)
    out["dense3"]["gflop"] = 3 * 2.0 * B * N * H / 1e9
    out["sparse_gflop"] = 2 * 4.0 * H * out["entries_per_batch"] / 1e9 + 2.0 * H * out["entries_per_batch"] / 1e9
    out["dense3_over_step"] = out["dense3"]["ms"] / out["step"]["ms"]
    out["adam_share_of_step"] = out["adam"]["ms"] / out["step"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="user-ml1m,item-ml1m,user-ml20m")
    args = ap.parse_args()
    ctx = ops.get_context(0)
    res = {"bench": "autorec", "arch": ctx.arch, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "shapes": {s: run_shape(ctx, s, args.steps, args.warmup, args.reps) for s in args.shapes.split(",")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "autorec_bench.jsonl"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
