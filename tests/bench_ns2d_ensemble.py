#!/usr/bin/env python
"""Cost of per-sample parameters (tcfd_ns2d_plan_set_ensemble, k_cols<..., ENS = 1>): ms per RK4-CN step of a WHOLE ensemble of B
members with their own viscosity, drag and forcing amplitude,
    (a) ensemble   one call of one ensemble operator;
    (b) scalar     the scalar operator (one physics) on the same batch -- the difference to (a) is the cost of the feature; the
                   bytes model says 1.00 (three uniform loads per workgroup, one multiply-subtract per table entry, no bytes);
    (c) per_member what a user did before: B scalar operators, one batch-1 call each,
the three alternating inside one process; median and spread (max - min) of five regions timed with device events after a
warm-up (the protocol of tests/bench_ns2d_jvp.py).  After the regions, the library's per-launch events split (a) and (b) by
kernel kind (`kernel_ms_per_step`): where a difference between the two sits; and ONE plan and workspace (the scalar operator's) is
timed with the mode switched on and off in alternation (`same_plan_*`): the ENS = 1 kernels against the ENS = 0 kernels with
nothing else different.

    python tests/bench_ns2d_ensemble.py [--regions 5] [--steps K] [--only n,B,f64] [--json profiles/ns2d_ensemble_bench.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch_cfd_amd as tc  # noqa: E402

L = 2 * math.pi
CONFIGS = ((256, 16, "f32"), (1024, 16, "f64"), (1024, 16, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}


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


KINDS = {0: "cols_A", 1: "rows_advect", 2: "cols_CA", 3: "cols_C", 5: "other"}


def kernel_split(op, w0, dt, K):
    """ms per step by kernel kind, from the library's per-launch events (tcfd_ns2d_profile_begin / _end) around one call."""
    lib, plan = tc._lib.load(), op._plan(w0)
    max_rec = K * 64 * 16 + 64
    cnt, kinds, ms = ctypes.c_int(0), (ctypes.c_int * max_rec)(), (ctypes.c_float * max_rec)()
    tc._lib.check(lib.tcfd_ns2d_profile_begin(plan.handle, max_rec), "profile_begin")
    op._fused_steps(w0, dt, K, want_dwdt=False)
    torch.cuda.synchronize()
    tc._lib.check(lib.tcfd_ns2d_profile_end(plan.handle, max_rec, ctypes.byref(cnt), kinds, ms), "profile_end")
    out = {}
    for i in range(min(cnt.value, max_rec)):
        name = KINDS.get(kinds[i], str(kinds[i]))
        out[name] = out.get(name, 0.0) + ms[i] / K
    return {k: round(v, 5) for k, v in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="steps per library call (0: 20 at 256, 5 at 1024)")
    ap.add_argument("--only", default=None, help="n,B,f64|f32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns2d_ensemble.py measures on a HIP device; none is visible")
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
        nus = [1e-3 * (1 + b) for b in range(B)]
        drags = [0.1 + 0.01 * b for b in range(B)]
        scales = [1.0 + 0.1 * b for b in range(B)]

        def make(nu, drag, **kw):
            return tc.NavierStokes2DSpectral(nu, grid, drag=drag, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper(), **kw).to(dev)

        ens = make(nus, drags, forcing_scale=scales)
        scalar = make(1e-3, 0.1)
        members = [make(nus[b], drags[b]) for b in range(B)]
        dt = tc.stable_time_step(dx=L / n, max_velocity=5.0, max_courant_number=0.5, viscosity=1e-3)
        gen = torch.Generator().manual_seed(n + B)
        w0 = torch.fft.rfft2(torch.randn(B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev))
        k2 = (scalar.kx**2 + scalar.ky**2) * L * L
        w0 = (w0 * torch.exp(-k2 / 64.0)).contiguous()          # a smooth state of moderate amplitude
        singles = [w0[b:b + 1].contiguous() for b in range(B)]
        K = args.steps or (20 if n <= 256 else 5)

        def run_ensemble():
            ens._fused_steps(w0, dt, K, want_dwdt=False)

        def run_scalar():
            scalar._fused_steps(w0, dt, K, want_dwdt=False)

        def run_members():
            for op, w in zip(members, singles):
                op._fused_steps(w, dt, K, want_dwdt=False)

        variants = [("ensemble", run_ensemble, 4), ("scalar", run_scalar, 4), ("per_member", run_members, 2)]
        for _, fn, _ in variants:   # warm-up: plans, code objects, workspaces
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps in variants:
                times[name].append(region(fn, reps) / K)
        a, b_, c = (stats(times[k]) for k in ("ensemble", "scalar", "per_member"))
        info = ens._plan(w0).info()
        row = {"n": n, "batch": B, "dtype": tag, "steps_per_call": K, "regions": args.regions, "plan": info,
               "ensemble_ms": a, "scalar_same_batch_ms": b_, "per_member_calls_ms": c,
               "ensemble_over_scalar": a["median_ms"] / b_["median_ms"],
               "ensemble_over_scalar_exceeds_1_by_more_than_spread": bool(
                   a["median_ms"] - b_["median_ms"] > max(a["spread_ms"], b_["spread_ms"])),
               "speedup_vs_per_member_calls": c["median_ms"] / a["median_ms"],
               # the bar: one ensemble call beats B batch-1 calls by more than the spread of the regions
               "beats_per_member_calls_by_more_than_spread": bool(
                   c["median_ms"] - a["median_ms"] > max(a["spread_ms"], c["spread_ms"]))}
        # where a difference between (a) and (b) sits: event time per kernel kind, the median of three instrumented calls each
        split = {}
        for name, op in (("ensemble", ens), ("scalar", scalar)):
            runs = [kernel_split(op, w0, dt, K) for _ in range(3)]
            split[name] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        row["kernel_ms_per_step"] = split
        # (a) and (b) are two operators: two plans, two workspaces.  The member arithmetic ALONE: the scalar operator's own plan
        # and workspace with the mode switched on (every member = the scalar's values: the same flow) and off, alternating
        plan = scalar._plan(w0)
        on, off = [], []
        for _ in range(args.regions):
            plan.set_ensemble(scalar.laplace, [1e-3] * B, [0.1] * B, [1.0] * B)
            run_scalar()
            on.append(region(run_scalar, 4) / K)
            plan.set_ensemble(None, [], [], [])
            run_scalar()
            off.append(region(run_scalar, 4) / K)
        row["same_plan_mode_on_ms"], row["same_plan_mode_off_ms"] = stats(on), stats(off)
        row["same_plan_on_over_off"] = row["same_plan_mode_on_ms"]["median_ms"] / row["same_plan_mode_off_ms"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ens, scalar, members, w0, singles
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
