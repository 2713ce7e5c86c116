#!/usr/bin/env python
"""A Reynolds-number sweep as ONE ensemble: Kolmogorov-forced flows that share the grid, the forcing and the initial vorticity and
differ in viscosity -- one `NavierStokes2DSpectral` with a per-sample `viscosity`, one fused library call per block of steps for
all members (instead of one operator and one batch-1 call per viscosity).  Prints each member's enstrophy at the end.

    python examples/ns2d_reynolds_sweep.py [--n 256] [--members 8] [--steps 2000]
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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--steps", type=int, default=2000)
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda:0")
    n, B, L = args.n, args.members, 2 * math.pi
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    nus = [1e-2 * 10 ** (-2 * b / max(B - 1, 1)) for b in range(B)]      # 1e-2 ... 1e-4, evenly in the logarithm
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False)
    op = tc.NavierStokes2DSpectral(viscosity=nus, grid=grid, drag=0.1, smooth=True, forcing_fn=forcing,
                                   solver=tc.RK4CrankNicolsonStepper()).to(dev)
    dt = tc.stable_time_step(dx=L / n, max_velocity=7.0, max_courant_number=0.5, viscosity=min(nus))
    w = vorticity_field(grid, 4, batch_seeds=[0], device=dev)           # the same initial condition for every member
    w_hat = tc.fft_plan(n, torch.complex128, dev).rfft2(w).expand(B, -1, -1).contiguous()
    with torch.no_grad():
        done = 0
        while done < args.steps:
            k = min(200, args.steps - done)
            w_hat, _ = op(w_hat, dt, steps=k)
            done += k
    # enstrophy 1/2 <w^2> by Parseval on the half spectrum (interior columns count twice)
    weight = torch.full((n // 2 + 1,), 2.0, device=dev)
    weight[0] = weight[-1] = 1.0
    enstrophy = 0.5 * ((w_hat.abs() ** 2) * weight).sum(dim=(-2, -1)) / float(n) ** 4
    print(f"n = {n}, {B} members, {args.steps} steps of dt = {dt:.3e} (t = {args.steps * dt:.2f})")
    for nu, z in zip(nus, enstrophy.tolist()):
        print(f"  nu = {nu:.3e}   Re ~ {1.0 / nu:9.1f}   enstrophy = {z:.6e}")
    assert bool(torch.isfinite(enstrophy).all())


if __name__ == "__main__":
    main()
