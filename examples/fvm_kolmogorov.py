#!/usr/bin/env python
"""Kolmogorov-forced turbulence on the finite-volume (MAC grid) solver: the reference's notebook
examples/Kolmogrov2d_rk4_fvm_forced_turbulence.ipynb end to end -- n = 256, fp64, seed 42, max velocity 3, classic RK4,
2 000 steps recorded every 20, vorticity by the forward-difference curl.

    python examples/fvm_kolmogorov.py [--out traj.pt]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.initial_conditions import curl_2d, filtered_velocity_field  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="save (ux, uy, vorticity) trajectories with torch.save")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    n, diam, viscosity, max_velocity, peak_wavenumber = 256, 2 * math.pi, 1e-3, 3.0, 3.0
    inner_steps, outer_steps = 20, 100
    grid = tc.Grid((n, n), domain=((0, diam), (0, diam)))
    v0 = filtered_velocity_field(grid, max_velocity, peak_wavenumber, iterations=3, random_state=42, device="cuda")
    dt = tc.stable_time_step(dx=min(grid.step), max_velocity=max_velocity, max_courant_number=0.5, viscosity=viscosity)
    step_fn = tc.RKStepper.from_method(method="classic_rk4", requires_grad=False)
    forcing_fn = tc.KolmogorovForcing(diam=diam, wave_number=peak_wavenumber, grid=grid, offsets=grid.cell_faces)
    ns2d = tc.NavierStokes2DFVMProjection(viscosity=viscosity, grid=grid, density=1.0, drag=0.1, forcing=forcing_fn,
                                          solver=step_fn)
    with torch.no_grad():
        ux, uy = tc.get_trajectory_fvm(ns2d, v0, dt, num_steps=inner_steps * outer_steps, record_every_steps=inner_steps)
        w = curl_2d((ux, uy), grid)
    print(f"dt = {dt}, {outer_steps} records of {inner_steps} steps; finite: {bool(torch.isfinite(w).all())}; "
          f"max |u| at the end = {torch.sqrt(ux[-1] ** 2 + uy[-1] ** 2).max().item():.3f}")
    if args.out:
        torch.save({"ux": ux.cpu(), "uy": uy.cpu(), "vorticity": w.cpu(), "dt": dt}, args.out)


if __name__ == "__main__":
    main()
