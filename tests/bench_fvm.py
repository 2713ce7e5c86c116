#!/usr/bin/env python
"""Throughput of the finite-volume step (tcfd_fvm.hip): steps/s, algorithmic GB/s and fraction of 8 TB/s on the pass
model below, next to the plain-torch restatement tests/fvm_ops.py on the same GPU.

    python tests/bench_fvm.py [--steps K] [--warmup W] [--json out.json]

Pass model (S = B n^2 w bytes, one real field; w = 8 fp64, 4 fp32), per RK stage of the shipped launch sequence:
    apply u_i = u*_i - grad q        read u*, q, write u_i      5S   (stages > 0 and the step's result)
    stage kernel                     read u_i (2S), u0 (2S), read + write the targets it updates (4S per target)
    divergence                       read u*, write div         3S
    rfft2 / x inverse / irfft2       ~ 2.5S + 2 x 1.1S + 2.5S   (half spectrum = 1.03 S; the transforms' own passes)
The fused target design (divergence in the row pass, multiply in the column pass, gradient in the stage load) is the
issue's 18S per stage = 72S per classic-RK4 step; the fraction below uses that 72S model as the algorithmic byte count.
"""
import argparse
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fvm_ops as F  # noqa: E402
import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd import initial_conditions as ic  # noqa: E402

PEAK = 8e12
L = 2 * math.pi
CONFIGS = ((256, 1, torch.float64), (1024, 16, torch.float64), (1024, 64, torch.float64), (1024, 64, torch.float32))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n, B, dtype in CONFIGS:
        torch.set_default_dtype(dtype)
        grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
        ux, uy = ic.filtered_velocity_field(grid, 3.0, 3.0, random_state=0, device=dev, batch_seeds=list(range(B)))
        forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=3, offsets=grid.cell_faces)
        eq = tc.NavierStokes2DFVMProjection(1e-3, grid, drag=0.1, forcing=forcing,
                                            solver=tc.RKStepper.from_method(method="classic_rk4"))
        dt = tc.stable_time_step(dx=L / n, max_velocity=3.0, max_courant_number=0.5, viscosity=1e-3)
        state = [(ux, uy)]
        with torch.no_grad():
            def hip():
                state[0] = eq(state[0], dt, steps=1)
            t_hip = timed(hip, args.steps, args.warmup)
            a, b = eq.solver.weights(dt)
            force = tuple(f.to(dev, dtype) for f in F.kolmogorov_staggered(n, 3))
            inv = F.inverse_eigenvalues(n, L / n, dtype).to(dev)
            ref = [(ux, uy)]

            def ops():
                ref[0] = F.step(ref[0][0], ref[0][1], dt, a, b, L / n, 1e-3, 0.1, force, inv)
            t_ops = timed(ops, args.torch_steps, 1)
        S = B * n * n * (8 if dtype == torch.float64 else 4)
        gbs = 72 * S / t_hip / 1e9
        row = {"n": n, "batch": B, "dtype": str(dtype).replace("torch.", ""), "steps_per_s": 1 / t_hip,
               "ms_per_step": t_hip * 1e3, "model_bytes_per_step": 72 * S, "algorithmic_GBps": gbs,
               "fraction_of_8TBps": gbs * 1e9 / PEAK, "torch_ops_steps_per_s": 1 / t_ops, "speedup_vs_torch_ops": t_ops / t_hip}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del state, ref, eq, ux, uy
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
