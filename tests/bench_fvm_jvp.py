#!/usr/bin/env python
"""Throughput of the tangent-linear finite-volume step (k_fvm_stage_jvp on a tangent plan, tcfd_fvm_plan_set_tangent): ms per
classic-RK4 step of ``tangent_step`` next to the plain step of the same equation (k_fvm_stage, untouched by the tangent) and to
torch.autograd.forward_ad through the plain-torch restatement tests/fvm_ops.py on the same GPU, the three alternating inside
one process; median and spread (max - min) of five regions timed with device events after a warm-up.

    python tests/bench_fvm_jvp.py [--regions 5] [--steps K] [--no-torch] [--only n,B,f64] [--schemes van_leer,upwind] [--json out.json]

Pass model (S = B n^2 w bytes, one real field of the batch of B states).  A tangent plan runs every pass of the shipped
sequence over 2 B fields -- copies, k_fvm_div, the transforms, k_fvm_mul, k_fvm_apply -- and the stage kernel once over B
samples with both halves of every operand, minus the state stencil that the tangent shares with the state: a time ratio of
2.0 to the plain step on bytes alone.  The algorithmic byte count is twice that of tests/bench_fvm.py, 2 x 72 S per step.
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

import fvm_jvp_ops as J  # noqa: E402
import fvm_schemes_ops as S  # noqa: E402
import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd import initial_conditions as ic  # noqa: E402

PEAK = 8e12
CONFIGS = ((256, 1, "f64"), (1024, 16, "f64"), (1024, 16, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
MODEL_S, PLAIN_S = 144, 72


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="steps per library call (0: 20 at 256, 5 at 1024)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward AD (profiling runs)")
    ap.add_argument("--only", default=None, help="n,B,f64|f32")
    ap.add_argument("--schemes", default="van_leer", help="comma-separated advection schemes, or all")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fvm_jvp.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), t_),)
    schemes = S.SCHEMES if args.schemes == "all" else tuple(args.schemes.split(","))
    rows = []
    for scheme in schemes:
        for n, B, tag in configs:
            real = REAL[tag]
            torch.set_default_dtype(torch.float64)
            ph = S.Physics(scheme, n, wave=4)
            eq = ph.equation(tc.RKStepper.from_method(method="classic_rk4"))
            dt = tc.stable_time_step(dx=ph.h, max_velocity=2.0, max_courant_number=0.5, viscosity=ph.nu)
            a, b = eq.solver.weights(dt)
            u = tuple(c.detach().to(real).contiguous() for c in
                      ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=dev, batch_seeds=list(range(B))))
            du = tuple(1e-3 * torch.roll(c, (1, 3), (-2, -1)) for c in u)
            K = args.steps or (20 if n <= 256 else 5)
            ops_step = ph.rollout(a, b, dt, 1, dev, real)

            def tangent():
                eq.tangent_step(u, du, dt, K)

            def plain():
                eq(u, dt, K)

            def torch_ops():
                J.jvp(ops_step, u, du)

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
            field = B * n * n * (8 if tag == "f64" else 4)
            tan, pl = stats(times["tangent"]), stats(times["plain"])
            gbs = MODEL_S * field / (tan["median_ms"] / 1e3) / 1e9
            row = {"scheme": scheme, "n": n, "batch": B, "dtype": tag, "steps_per_call": K, "regions": args.regions,
                   "tangent_step_ms": tan, "plain_step_ms": pl, "tangent_over_plain": tan["median_ms"] / pl["median_ms"],
                   "expected_on_bytes": MODEL_S / PLAIN_S, "model_bytes_per_step": MODEL_S * field, "algorithmic_GBps": gbs,
                   "fraction_of_8TBps": gbs * 1e9 / PEAK}
            if not args.no_torch:
                ops = stats(times["torch_ops_forward_ad"])
                row["torch_ops_forward_ad_ms"] = ops
                row["speedup_vs_torch_ops"] = ops["median_ms"] / tan["median_ms"]
                # the bar: faster than the torch-op forward AD by more than the spread of the regions
                row["beats_torch_ops_by_more_than_spread"] = bool(
                    ops["median_ms"] - tan["median_ms"] > max(ops["spread_ms"], tan["spread_ms"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del eq, u, du, ops_step
            torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
