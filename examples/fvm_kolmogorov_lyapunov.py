#!/usr/bin/env python
"""Leading Lyapunov exponent of the finite-volume (MAC grid) Kolmogorov flow by Benettin's method on the tangent-linear step.

The flow is that of examples/fvm_kolmogorov.py (the reference's notebook: classic RK4 with a pressure projection per stage,
van Leer advection, Kolmogorov forcing k = 3, drag 0.1, nu = 1e-3, max velocity 3), at a smaller default size.  A velocity u and
a perturbation du are advanced together by ``tangent_step(u, du, dt, steps=K)`` -- K RK4 steps of the state and of its
tangent-linear model, all stages and projections, in one library call -- then the perturbation is renormalised and the logarithm
of its growth recorded.  The running mean of log(growth) / (K dt) converges to the leading exponent; the normalised perturbation
to the leading (backward) Lyapunov vector.

    python examples/fvm_kolmogorov_lyapunov.py [--n 64] [--spinup 1000] [--rounds 100] [--inner 20] [--batch 4]

The batch holds independent initial conditions: every sample gives its own estimate, their scatter a cheap error bar.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.initial_conditions import filtered_velocity_field  # noqa: E402


def norm(du):
    """L2 norm per sample of a velocity pair (up to the constant cell area)."""
    return (du[0].square().sum(dim=(-2, -1)) + du[1].square().sum(dim=(-2, -1))).sqrt()


def scaled(du, s):
    return tuple(c / s[:, None, None] for c in du)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--spinup", type=int, default=1000, help="steps of the plain solver before the measurement")
    ap.add_argument("--rounds", type=int, default=100, help="renormalisations")
    ap.add_argument("--inner", type=int, default=20, help="tangent steps between two renormalisations")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda:0")
    n, diam, viscosity, max_velocity, wave = args.n, 2 * math.pi, 1e-3, 3.0, 3.0
    grid = tc.Grid((n, n), domain=((0, diam), (0, diam)))
    forcing = tc.KolmogorovForcing(diam=diam, wave_number=wave, grid=grid, offsets=grid.cell_faces)
    eq = tc.NavierStokes2DFVMProjection(viscosity=viscosity, grid=grid, density=1.0, drag=0.1, forcing=forcing,
                                        solver=tc.RKStepper.from_method(method="classic_rk4"))
    dt = tc.stable_time_step(dx=min(grid.step), max_velocity=max_velocity, max_courant_number=0.5, viscosity=viscosity)
    seeds = list(range(args.batch))
    with torch.no_grad():
        u = filtered_velocity_field(grid, max_velocity, wave, iterations=3, random_state=42, device=dev, batch_seeds=seeds)
        u = eq(u, dt, steps=args.spinup)             # onto the attractor
        du = filtered_velocity_field(grid, 1.0, 2 * wave, iterations=3, random_state=7, device=dev,
                                     batch_seeds=[100 + s for s in seeds])
        du = eq.pressure_projection(du)              # (the filtered field is divergence-free already, up to roundoff)
    du = scaled(du, norm(du))
    log_growth = torch.zeros(args.batch, dtype=torch.float64, device=dev)
    for r in range(1, args.rounds + 1):
        u, du = eq.tangent_step(u, du, dt, steps=args.inner)
        g = norm(du)
        log_growth += torch.log(g)
        du = scaled(du, g)
        if r % max(1, args.rounds // 10) == 0:
            lam = (log_growth / (r * args.inner * dt)).cpu()
            print(f"t = {r * args.inner * dt:8.3f}   lambda_1 per sample = {[round(v, 4) for v in lam.tolist()]}   "
                  f"mean {lam.mean().item():.4f}")
    lam = (log_growth / (args.rounds * args.inner * dt)).cpu()
    print(f"leading Lyapunov exponent after t = {args.rounds * args.inner * dt:.2f}: {lam.mean().item():.4f} "
          f"+- {lam.std().item() if args.batch > 1 else float('nan'):.4f} (scatter of {args.batch} samples); "
          f"state finite: {bool(torch.isfinite(u[0]).all() and torch.isfinite(u[1]).all())}")


if __name__ == "__main__":
    main()
