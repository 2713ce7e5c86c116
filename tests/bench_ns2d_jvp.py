#!/usr/bin/env python
"""Throughput of the tangent-linear spectral step (tcfd_ns2d_step_jvp, k_rows_jvp): ms per RK4-CN step of ``tangent_step``
next to the plain fused step of the same operator and to torch.autograd.forward_ad through the plain-torch restatement
tests/ns2d_ops.py on the same GPU, the three alternating inside one process; median and spread (max - min) of five regions
timed with device events after a warm-up.

    python tests/bench_ns2d_jvp.py [--regions 5] [--steps K] [--no-torch] [--only n,B,f64] [--json out.json]

Pass model (S = B n m 2w bytes, one complex half-spectrum field; what each launch must read and write once):
    per stage   2 x k_cols<MODE_A>   (w -> 4 planes, dw -> 4 planes)          2 x 5 S
                k_rows_jvp           (8 planes in, p and dp out)               10 S   (two row passes: + 4 S re-read)
                2 x k_cols<MODE_F>   (p -> F, dp -> dF)                        2 x 2 S
                k_stage_update_jvp   (F dF h dh b db in, h dh u du out)        10 S   (8 S at the first and the last stage)
    RK4-CN step (5 stages)           5 x 34 S - 4 S = 166 S                    (plain fused step: 70 S)
Expected time ratio to the plain step on bytes alone: 166 / 70 = 2.4 -- twice the advection traffic (2 x 25 S per stage pair
against 2 x 14 S fused) plus the stage updates and closing passes that the plain step fuses into its column kernels.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ns2d_ops  # noqa: E402
import torch_cfd_amd as tc  # noqa: E402

PEAK = 8e12
L = 2 * math.pi
CONFIGS = ((256, 16, "f64"), (1024, 16, "f64"), (1024, 16, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
MODEL_S, PLAIN_S = 166, 70
TWO_PASS_EXTRA_S = 5 * 4


def region(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / reps


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "spread_ms": (max(ts) - min(ts)) * 1e3}


def two_pass(n, tag):
    """Sizes whose row pass runs as two launches (csrc/tcfd_ns2d.hip, jvp_two_pass)."""
    return tag == "f64" and n in (80, 160, 320, 640, 1280)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="steps per library call (0: 20 at 256, 5 at 1024)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward AD (profiling runs)")
    ap.add_argument("--only", default=None, help="n,B,f64|f32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns2d_jvp.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), t_),)
    rows = []
    for n, B, tag in configs:
        real = REAL[tag]
        torch.set_default_dtype(real)
        grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
        forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
        op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
        dt = tc.stable_time_step(dx=L / n, max_velocity=5.0, max_courant_number=0.5, viscosity=1e-3)
        gen = torch.Generator().manual_seed(n + B)
        w0 = torch.fft.rfft2(torch.randn(B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev))
        k2 = (op.kx**2 + op.ky**2) * L * L
        w0 = w0 * torch.exp(-k2 / 64.0)          # a smooth state of moderate amplitude
        dw = torch.roll(w0, 1, 0) * 1e-3
        K = args.steps or (20 if n <= 256 else 5)
        t = ns2d_ops.tables(n, "kolmogorov", True, real=real, device=dev)
        sched = ns2d_ops.schedule(op.solver, dt)

        def tangent():
            op.tangent_step(w0, dw, dt, K)

        def plain():
            op(w0, dt, K)

        def torch_ops():
            ns2d_ops.jvp(lambda w: ns2d_ops.advance(w, t, sched, 1), w0, dw)

        variants = [("tangent", tangent, 2, K), ("plain", plain, 4, K)]
        if not args.no_torch:
            variants.append(("torch_ops_forward_ad", torch_ops, 1, 1))
        for _, fn, _, _ in variants:   # warm-up: code objects, workspaces, library algorithm choices
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps, per in variants:
                times[name].append(region(fn, reps) / per)
        S = B * n * (n // 2 + 1) * 2 * (8 if tag == "f64" else 4)
        model = MODEL_S + (TWO_PASS_EXTRA_S if two_pass(n, tag) else 0)
        tan, pl = stats(times["tangent"]), stats(times["plain"])
        gbs = model * S / (tan["median_ms"] / 1e3) / 1e9
        row = {"n": n, "batch": B, "dtype": tag, "steps_per_call": K, "regions": args.regions,
               "tangent_step_ms": tan, "plain_step_ms": pl, "row_pass": "two passes" if two_pass(n, tag) else "one pass",
               "tangent_over_plain": tan["median_ms"] / pl["median_ms"], "expected_on_bytes": model / PLAIN_S,
               "model_bytes_per_step": model * S, "algorithmic_GBps": gbs, "fraction_of_8TBps": gbs * 1e9 / PEAK}
        if not args.no_torch:
            ops = stats(times["torch_ops_forward_ad"])
            row["torch_ops_forward_ad_ms"] = ops
            row["speedup_vs_torch_ops"] = ops["median_ms"] / tan["median_ms"]
            # the bar: faster than the torch-op forward AD by more than the spread of the regions
            row["beats_torch_ops_by_more_than_spread"] = bool(
                ops["median_ms"] - tan["median_ms"] > max(ops["spread_ms"], tan["spread_ms"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del op, w0, dw, t
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
