#!/usr/bin/env python
"""Recover an initial vorticity field from one observation 50 steps later (the inverse problem at the core of 4D-Var) with the
adjoint model of the fused spectral step and ``torch.optim.LBFGS`` -- no autograd graph anywhere.

The misfit J(w0) = 1/2 sum |M(w0) - obs|^2 over the half spectrum (M = 50 RK4-CN steps) has the gradient M'(w0)^T (M(w0) - obs):
one plain fused forward for the residual, then ``op.adjoint_step(w0, residual, dt, steps)`` -- the fused forward once per step
into the saved buffer and ONE library call (tcfd_ns2d_step_vjp) that reverses all steps.  ``--checkpoint c`` keeps every c-th
step input only (steps / c + c fields instead of steps; the same bits).  64 x 64, fp64, Kolmogorov forcing k = 4, on generated data.

    python examples/ns2d_fit_initial_condition.py [--n 64] [--steps 50] [--iters 30] [--checkpoint 1]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.initial_conditions import vorticity_field  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=30, help="outer L-BFGS iterations")
    ap.add_argument("--checkpoint", type=int, default=1, help="keep every c-th step input (adjoint_step's checkpoint_every)")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda:0")
    n, diam, steps = args.n, 2 * math.pi, args.steps
    grid = tc.Grid(shape=(n, n), domain=((0, diam), (0, diam)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
    op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    dt = tc.stable_time_step(dx=diam / n, max_velocity=7.0, max_courant_number=0.5, viscosity=1e-3)
    plan = tc.fft_plan(n, torch.complex128, dev, diam=diam)
    truth = plan.rfft2(vorticity_field(grid, 4, device=dev, batch_seeds=[0]))
    obs = op(truth, dt, steps=steps)[0]                                       # the observation, 50 steps later
    guess = plan.rfft2(vorticity_field(grid, 4, device=dev, batch_seeds=[1]))  # an unrelated field of the same spectrum
    p = torch.view_as_real(guess.clone()).requires_grad_(True)                # the control: Re / Im of the half spectrum
    opt = torch.optim.LBFGS([p], lr=1.0, max_iter=args.iters, history_size=20, line_search_fn="strong_wolfe",
                            tolerance_grad=1e-12, tolerance_change=1e-14)
    calls = [0]

    def misfit_and_gradient():
        w0 = torch.view_as_complex(p.detach())
        residual = op(w0, dt, steps=steps)[0] - obs
        _, wbar = op.adjoint_step(w0, residual, dt, steps=steps, checkpoint_every=args.checkpoint)
        return 0.5 * residual.abs().pow(2).sum(), wbar

    def closure():
        J, wbar = misfit_and_gradient()
        p.grad = torch.view_as_real(wbar).clone()
        calls[0] += 1
        if calls[0] == 1 or calls[0] % 5 == 0:
            err = (torch.linalg.norm(torch.view_as_complex(p.detach()) - truth) / torch.linalg.norm(truth)).item()
            print(f"evaluation {calls[0]:3d}: misfit {J.item():.6e}   |w0 - truth| / |truth| = {err:.3e}")
        return J

    J0, _ = misfit_and_gradient()
    opt.step(closure)
    J1, _ = misfit_and_gradient()
    err = (torch.linalg.norm(torch.view_as_complex(p.detach()) - truth) / torch.linalg.norm(truth)).item()
    print(f"misfit {J0.item():.3e} -> {J1.item():.3e} in {calls[0]} evaluations of ({steps} steps forward + the adjoint model); "
          f"initial condition recovered to {err:.3e} (relative L2 over the half spectrum)")


if __name__ == "__main__":
    main()
