#!/usr/bin/env python
"""Forward + backward throughput of the finite-volume solver (tcfd_fvm.hip adjoint kernels, torch_cfd_amd/fvm_autograd.py):
steps/s of a K-step classic-RK4 rollout and its gradient with respect to the initial velocity, next to the forward-only
rate and to torch autograd through the plain-torch restatement tests/fvm_ops.py on the same GPU; peak device memory of
the forward + backward; algorithmic GB/s and fraction of 8 TB/s on the pass model below.

    python tests/bench_fvm_grad.py [--steps K] [--reps R] [--torch-steps K2] [--no-torch] [--json out.json]

Pass model, counted as tests/bench_fvm.py counts the forward (S = B n^2 w bytes, one real field; 18 S per RK stage of the
fused-target design, 72 S per classic-RK4 step): a forward + backward step is the forward (72 S), the recomputation of
the stage states u_1 .. u_3 (3 stages, 54 S) and four reverse stages (gather VJP, projection of its result, RK
bookkeeping: 18 S each, 72 S), 198 S in all.
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
CONFIGS = ((256, 1, torch.float64), (1024, 16, torch.float64), (1024, 16, torch.float32))
MODEL_S = 72 + 3 * 18 + 4 * 18   # per forward + backward classic-RK4 step


def timed(fn, reps, warmup):
    """Seconds per call of fn (device events around reps calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / reps


def dot(u, cot):
    return (u[0] * cot[:, 0]).sum() + (u[1] * cot[:, 1]).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="rollout length K of the HIP forward + backward")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-steps", type=int, default=1, help="rollout length of the torch-ops forward + backward")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops baseline (profiling runs)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = args.steps
    rows = []
    for n, B, dtype in CONFIGS:
        torch.set_default_dtype(dtype)
        grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
        ux, uy = ic.filtered_velocity_field(grid, 3.0, 3.0, random_state=0, device=dev, batch_seeds=list(range(B)))
        ux, uy = ux.detach(), uy.detach()
        forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=3, offsets=grid.cell_faces)
        eq = tc.NavierStokes2DFVMProjection(1e-3, grid, drag=0.1, forcing=forcing,
                                            solver=tc.RKStepper.from_method(method="classic_rk4"))
        dt = tc.stable_time_step(dx=L / n, max_velocity=3.0, max_courant_number=0.5, viscosity=1e-3)
        cot = torch.randn(B, 2, n, n, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev, dtype)

        def forward_only():
            with torch.no_grad():
                eq((ux, uy), dt, steps=K)

        def hip_grad():
            u = (ux.clone().requires_grad_(), uy.clone().requires_grad_())
            torch.autograd.grad(dot(eq(u, dt, steps=K), cot), u)

        t_fwd = timed(forward_only, args.reps, args.warmup) / K
        t_grad = timed(hip_grad, args.reps, args.warmup) / K
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        hip_grad()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        S = B * n * n * (8 if dtype == torch.float64 else 4)
        gbs = MODEL_S * S / t_grad / 1e9
        row = {"n": n, "batch": B, "dtype": str(dtype).replace("torch.", ""), "rollout_steps": K,
               "fwd_bwd_steps_per_s": 1 / t_grad, "fwd_bwd_ms_per_step": t_grad * 1e3,
               "forward_only_steps_per_s": 1 / t_fwd, "fwd_bwd_over_forward_time": t_grad / t_fwd,
               "peak_bytes_fwd_bwd": peak, "saved_inputs_bytes": K * 2 * S,
               "model_bytes_per_step": MODEL_S * S, "algorithmic_GBps": gbs, "fraction_of_8TBps": gbs * 1e9 / PEAK}
        if not args.no_torch:
            a, b = eq.solver.weights(dt)
            force = tuple(f.to(dev, dtype) for f in F.kolmogorov_staggered(n, 3))
            inv = F.inverse_eigenvalues(n, L / n, dtype).to(dev)

            def ops_grad():
                u = (ux.clone().requires_grad_(), uy.clone().requires_grad_())
                v = u
                for _ in range(args.torch_steps):
                    v = F.step(v[0], v[1], dt, a, b, L / n, 1e-3, 0.1, force, inv)
                torch.autograd.grad(dot(v, cot), u)
            try:
                t_ops = timed(ops_grad, 1, 1) / args.torch_steps
                row.update({"torch_ops_fwd_bwd_steps_per_s": 1 / t_ops, "speedup_vs_torch_ops": t_ops / t_grad,
                            "torch_ops_rollout_steps": args.torch_steps})
            except torch.cuda.OutOfMemoryError:
                row["torch_ops_fwd_bwd_steps_per_s"] = "out of memory"
        rows.append(row)
        print(json.dumps(row), flush=True)
        del eq, ux, uy, cot
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
