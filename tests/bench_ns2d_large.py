#!/usr/bin/env python
"""The fused RK4-CN step at 4096^2 next to 2048^2 at the same number of points: ms per step of ``forward(w, dt, steps=K)`` and
of the same step in plain torch ops on the same GPU (tests/ns2d_ops.py ``advance`` on the device), the variants alternating
inside one process; median and spread (max - min) of five regions timed with device events after a warm-up.

    python tests/bench_ns2d_large.py [--regions 5] [--steps 2] [--only n,B,f64] [--no-dense] [--no-variants] [--json profiles/ns2d_large_bench.json]

Shapes: 4096^2 x 4 and 2048^2 x 16, fp64 and fp32.  At 4096^2 two more plans of the same operator run in the alternation, for
the choices csrc/tcfd_ns2d.hip makes at this size: TCFD_CHUNK=1 (one field per chunk, the policy of 2048^2, instead of four --
at B = 4 the whole batch in every launch) and TCFD_SPLIT=0 (whole-column tiles of one fp64 / two fp32 columns instead of the 2048-point halves).  The route a 4096
grid took before it was a fused size -- TensorOpPlan(DenseDft(4096)): dense 4096 x 4096 DFT matrices through matmul -- runs
ONCE, outside the alternation, at B = 1 for one step; its ratio is reported only.

Bytes model: 70 S per RK4-CN step, S = B n m 2w bytes = one complex half-spectrum field.  The share of
8 TB/s on that model is printed for both sizes from the same run.

The bar: at 4096^2 x 4 the fused step is faster than the torch-op step by more than the spread of the regions.
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
CONFIGS = ((4096, 4, "f64"), (2048, 16, "f64"), (4096, 4, "f32"), (2048, 16, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
MODEL_S = 70


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


def build(n, dev, env=None):
    """One operator; `env`: plan-time switches (read once, when the plan is created by the first call)."""
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
    op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        op._plan(torch.zeros(1, dtype=torch.complex128 if torch.get_default_dtype() == torch.float64 else torch.complex64,
                             device=dev))
    finally:
        for k in env or {}:
            del os.environ[k]
    return op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2, help="steps per library call")
    ap.add_argument("--only", default=None, help="n,B,f64|f32")
    ap.add_argument("--no-dense", action="store_true", help="skip the dense-transform route at 4096")
    ap.add_argument("--no-variants", action="store_true", help="skip the TCFD_CHUNK=1 / TCFD_SPLIT=0 plans at 4096")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-op step (profiling runs)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns2d_large.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), t_),)
    rows = []
    K = args.steps
    for n, B, tag in configs:
        real = REAL[tag]
        torch.set_default_dtype(real)
        op = build(n, dev)
        dt = tc.stable_time_step(dx=L / n, max_velocity=5.0, max_courant_number=0.5, viscosity=1e-3)
        gen = torch.Generator(device=dev).manual_seed(n + B)
        w0 = torch.fft.rfft2(torch.randn(B, n, n, generator=gen, dtype=real, device=dev))
        k2 = (op.kx**2 + op.ky**2) * L * L
        w0 = (w0 * torch.exp(-k2 / 64.0)).contiguous()          # a smooth state of moderate amplitude
        t = ns2d_ops.tables(n, "kolmogorov", True, real=real, device=dev)
        sched = ns2d_ops.schedule(op.solver, dt)
        info = op._plan(w0).info()
        single = plain = None
        variants = [("fused", lambda op=op: op(w0, dt, K), 2, K)]
        if n == 4096 and not args.no_variants:
            single = build(n, dev, {"TCFD_CHUNK": "1"})
            plain = build(n, dev, {"TCFD_SPLIT": "0"})
            assert plain._plan(w0).info()["split"] == 0 and info["split"] == 1
            variants.append(("fused_one_field_chunks", lambda op=single: op(w0, dt, K), 2, K))
            variants.append(("fused_whole_column_tiles", lambda op=plain: op(w0, dt, K), 2, K))
        if not args.no_torch:
            variants.append(("torch_ops", lambda: ns2d_ops.advance(w0, t, sched, 1), 2, 1))
        for _, fn, _, _ in variants:   # warm-up: code objects, workspaces, library algorithm choices
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps, per in variants:
                times[name].append(region(fn, reps) / per)
        S = B * n * (n // 2 + 1) * 2 * (8 if tag == "f64" else 4)
        fused = stats(times["fused"])
        gbs = MODEL_S * S / (fused["median_ms"] / 1e3) / 1e9
        row = {"n": n, "batch": B, "dtype": tag, "steps_per_call": K, "regions": args.regions, "plan": info,
               "fused_step_ms": fused, "model_bytes_per_step": MODEL_S * S, "algorithmic_GBps": gbs,
               "fraction_of_8TBps": gbs * 1e9 / PEAK}
        for name in ("fused_one_field_chunks", "fused_whole_column_tiles"):
            if name in times:
                row[name + "_ms"] = stats(times[name])
        if not args.no_torch:
            ops = stats(times["torch_ops"])
            row["torch_ops_step_ms"] = ops
            row["speedup_vs_torch_ops"] = ops["median_ms"] / fused["median_ms"]
            # the bar: faster than the torch-op step by more than the spread of the regions
            row["beats_torch_ops_by_more_than_spread"] = bool(
                ops["median_ms"] - fused["median_ms"] > max(ops["spread_ms"], fused["spread_ms"]))
        if n == 4096 and not args.no_dense:
            # what a 4096 grid ran before it was a fused size: once, B = 1, one step (reported only)
            from torch_cfd_amd.mixed_radix import DenseDft, TensorOpPlan

            dense = TensorOpPlan(op, DenseDft(n, w0.dtype), dev, op.forcing_hat())
            sc = op._schedule(op.solver, op.solver.params, dt)
            one = lambda: dense.step(w0[:1], sc["beta"], sc["gdt"], sc["mu"], 1, 1 / dt, True)
            one()
            torch.cuda.synchronize()
            ms = region(one, 1) * 1e3
            fused1 = region(lambda: op(w0[:1], dt, 1), 2) * 1e3
            row["dense_dft_route_B1_one_step_ms"] = ms
            row["fused_B1_one_step_ms"] = fused1
            row["speedup_vs_dense_dft_route_B1"] = ms / fused1
            del dense
        rows.append(row)
        print(json.dumps(row), flush=True)
        variants.clear()
        single = plain = None
        del op, w0, t
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
