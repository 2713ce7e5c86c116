#!/usr/bin/env python
"""A small FNO-paper data set: Gaussian-random-field initial vorticity, SinCos forcing, IMEX order 2, saved as a .pt.

    python examples/fno_dataset.py [--out fnodata_small.pt] [--replicable-init]

The full-size file of the paper (``fnodata_extra_64x64_N1280_v1e-3_T50_steps100_alpha2.5_tau7.pt``) is
n = 256, 1280 samples in batches of 256, dt = 1e-3, 30000 warm-up + 20000 steps, a record every 200, subsample 4.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torch_cfd_amd.data_gen import generate_fno_dataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="fnodata_small.pt")
    ap.add_argument("--replicable-init", action="store_true")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)   # the drivers compute in float64 and store float32
    stats = {}
    data = generate_fno_dataset(n=128, total_samples=8, batch_size=4, dt=1e-3, warmup_steps=500, total_steps=1000,
                                record_every_steps=100, viscosity=1e-3, scale=0.1, alpha=2.5, tau=7.0,
                                replicable_init=args.replicable_init, random_state=1127825, subsample=2, path=args.out,
                                stats=stats)
    for key, value in data.items():
        print(f"{key:<14} {tuple(value.shape)} {value.dtype}")
    print(f"stepping {stats['stepping_s']:.2f} s, saved {args.out}")


if __name__ == "__main__":
    main()
