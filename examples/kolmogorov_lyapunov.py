#!/usr/bin/env python
"""Leading Lyapunov exponent of Kolmogorov-forced 2-D turbulence by Benettin's method on the tangent-linear step.

A state w and a perturbation dw are advanced together by ``tangent_step(w, dw, dt, steps=K)`` -- K RK4-CN steps of the state and
of its tangent-linear model in one library call -- then the perturbation is renormalised and the logarithm of its growth
recorded.  The running mean of log(growth) / (K dt) converges to the leading exponent; the normalised perturbation to the leading
(backward) Lyapunov vector.  128 x 128, fp64, Kolmogorov forcing k = 4, drag 0.1, nu = 1e-3, on generated data.

    python examples/kolmogorov_lyapunov.py [--n 128] [--spinup 2000] [--rounds 200] [--inner 20] [--batch 4]

The batch holds independent initial conditions: every sample gives its own estimate, their scatter a cheap error bar.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.initial_conditions import vorticity_field  # noqa: E402


def norm(dw_hat):
    """L2 norm per sample of the real field behind a half spectrum (up to the constant factor of the transform)."""
    weight = torch.full((dw_hat.shape[-1],), 2.0, dtype=dw_hat.real.dtype, device=dw_hat.device)
    weight[0] = weight[-1] = 1.0
    return ((dw_hat.abs() ** 2) * weight).sum(dim=(-2, -1)).sqrt()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--spinup", type=int, default=2000, help="steps of the plain fused solver before the measurement")
    ap.add_argument("--rounds", type=int, default=200, help="renormalisations")
    ap.add_argument("--inner", type=int, default=20, help="tangent steps between two renormalisations")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda:0")
    n, diam = args.n, 2 * math.pi
    grid = tc.Grid(shape=(n, n), domain=((0, diam), (0, diam)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
    op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    dt = tc.stable_time_step(dx=diam / n, max_velocity=7.0, max_courant_number=0.5, viscosity=1e-3)
    plan = tc.fft_plan(n, torch.complex128, dev, diam=diam)
    w = plan.rfft2(vorticity_field(grid, 4, device=dev, batch_seeds=list(range(args.batch))))
    with torch.no_grad():
        w, _ = op(w, dt, steps=args.spinup)          # onto the attractor
    dw = plan.rfft2(vorticity_field(grid, 8, device=dev, batch_seeds=[100 + s for s in range(args.batch)]))
    dw = dw / norm(dw)[:, None, None]
    log_growth = torch.zeros(args.batch, dtype=torch.float64, device=dev)
    for r in range(1, args.rounds + 1):
        w, dw = op.tangent_step(w, dw, dt, steps=args.inner)
        g = norm(dw)
        log_growth += torch.log(g)
        dw = dw / g[:, None, None]
        if r % max(1, args.rounds // 10) == 0:
            lam = (log_growth / (r * args.inner * dt)).cpu()
            print(f"t = {r * args.inner * dt:8.3f}   lambda_1 per sample = {[round(v, 4) for v in lam.tolist()]}   "
                  f"mean {lam.mean().item():.4f}")
    lam = (log_growth / (args.rounds * args.inner * dt)).cpu()
    print(f"leading Lyapunov exponent after t = {args.rounds * args.inner * dt:.2f}: {lam.mean().item():.4f} "
          f"+- {lam.std().item() if args.batch > 1 else float('nan'):.4f} (scatter of {args.batch} samples); "
          f"state finite: {bool(torch.isfinite(torch.view_as_real(w)).all())}")


if __name__ == "__main__":
    main()
