#!/usr/bin/env python
"""Write a random visual-feature folder for the ratings of config_files/attribute_sample/, so that
config_files/sample_vbpr_amd.yml runs: one `<item id>.npy` (fp32 vector, non-negative like CNN features behind a ReLU) per rated
item.  The folder is generated data and is not committed.

    python scripts/make_visual_sample.py [--dim 512] [--seed 42] [--out config_files/attribute_sample/visual_features]
"""
import argparse
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratings", default=os.path.join(REPO, "config_files", "attribute_sample", "dataset.tsv"))
    ap.add_argument("--out", default=os.path.join(REPO, "config_files", "attribute_sample", "visual_features"))
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    items = sorted({int(line.split("\t")[1]) for line in open(args.ratings) if line.strip()})
    os.makedirs(args.out, exist_ok=True)
    rs = np.random.RandomState(args.seed)
    for item in items:
        np.save(os.path.join(args.out, f"{item}.npy"), np.maximum(rs.standard_normal(args.dim), 0).astype(np.float32))
    print(f"wrote {len(items)} vectors of length {args.dim} to {args.out}")


if __name__ == "__main__":
    main()
