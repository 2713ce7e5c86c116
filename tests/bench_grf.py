#!/usr/bin/env python
"""Timing of the GRF initial-condition kernel (tcfd_grf.hip) next to the same result in torch ops on the same GPU
(``torch.fft.ifft2`` of the scaled noise -> real part -> stride -> ``torch.fft.rfft2``), and the stepping rate of
``generate_fno_dataset``.

    python tests/bench_grf.py [--json out.json]

Per shape: device events around one call, after a warm-up, median of five.  Algorithmic bytes of the fold = noise once +
table once + half spectrum written once, reported as a fraction of 8 TB/s.  The noise here is device noise (only the
kernel is timed; the seeded CPU draw of the module is host work of its own).
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.data_gen import generate_fno_dataset  # noqa: E402

PEAK = 8e12
SHAPES = ((2048, 256, 16), (256, 256, 256), (2048, 2048, 4))   # n0, n, batch


def median_ms(fn, warmup=2, repeats=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--dataset-steps", type=int, default=400)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_default_dtype(torch.float64)
    rows = []
    for n0, n, B in SHAPES:
        for normalize in (False, True):
            g = tc.GRF2d(n=n, alpha=2.5, tau=7.0, device=dev, dtype=torch.float64, normalize=normalize)
            noise = torch.randn(B, 2, n0, n0, device=dev)
            table = g._device_table(n0, torch.float64, dev)
            out = torch.empty(B, n, n // 2 + 1, dtype=torch.complex128, device=dev)
            st = n0 // n

            def hip():
                g._spectrum(noise, n, out)

            def ops():
                s = torch.fft.ifft2(table * torch.complex(noise[:, 0], noise[:, 1])).real
                if normalize:
                    s = s / torch.linalg.norm(s / n0, dim=(-1, -2), keepdim=True)
                return torch.fft.rfft2(s[..., ::st, ::st])

            hip()
            want = ops()
            err = (torch.linalg.norm(out - want) / torch.linalg.norm(want)).item()
            del want
            t_hip, t_ops = median_ms(hip), median_ms(ops)
            nbytes = 8 * (2 * B * n0 * n0 + n0 * n0 + 2 * B * n * (n // 2 + 1))
            row = {"n0": n0, "n": n, "batch": B, "normalize": normalize, "dtype": "float64", "hip_ms": t_hip, "torch_ops_ms": t_ops,
                   "speedup_vs_torch_ops": t_ops / t_hip, "algorithmic_bytes": nbytes, "algorithmic_GBps": nbytes / t_hip / 1e6,
                   "fraction_of_8TBps": nbytes / (t_hip * 1e-3) / PEAK, "rel_l2_vs_torch_ops": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del noise, out
            torch.cuda.empty_cache()
    # stepping phase of the generator: 256^2 x 64 samples, float64, SinCos-forced IMEX order 2
    half = args.dataset_steps // 2
    for _ in range(2):   # the first run builds the plans
        stats = {}
        generate_fno_dataset(256, 64, 64, 1e-3, half, half, max(half // 4, 1), random_state=0, subsample=4, device=dev,
                             stats=stats)
    row = {"generate_fno_dataset": {"n": 256, "samples": 64, "dtype": "float64", "steps": 2 * half, "stepping_s": stats["stepping_s"],
                                    "steps_per_s": 2 * half / stats["stepping_s"],
                                    "sample_steps_per_s": 64 * 2 * half / stats["stepping_s"], "setup_s": stats["setup_s"],
                                    "handover_tail_s": stats["handover_tail_s"]}}
    rows.append(row)
    print(json.dumps(row), flush=True)
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
