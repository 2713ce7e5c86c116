#!/usr/bin/env python
"""The K leading Lyapunov exponents and the Kaplan-Yorke dimension of Kolmogorov-forced 2-D turbulence: Benettin's method with
QR re-orthonormalisation on the tangent bundle.

A state w and K perturbations dW of it are advanced together by ``tangent_bundle_step(w, dW, dt, steps)`` -- the steps of the
state and of K copies of its tangent-linear model in one library call, the state's share of every stage done once -- then
``orthonormalize_tangents`` factors dW = Q R in the real-field inner product, Q replaces dW and log diag(R) is recorded.  The
running means of log R[k, k] / time converge to the exponents lambda_1 >= lambda_2 >= ..., Q to the backward Lyapunov vectors.
The Kaplan-Yorke dimension is j + (lambda_1 + ... + lambda_j) / |lambda_{j+1}| with j the last index whose partial sum is not
negative.  Same flow and defaults as examples/kolmogorov_lyapunov.py, which stops at lambda_1 (0.60 +- 0.12 there): 128 x 128,
fp64, Kolmogorov forcing k = 4, drag 0.1, nu = 1e-3, on generated data.

    python examples/kolmogorov_lyapunov_spectrum.py [--n 128] [--tangents 8] [--spinup 2000] [--rounds 200] [--inner 20] [--batch 4]

The batch holds independent initial conditions: every sample gives its own spectrum, their scatter a cheap error bar.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.initial_conditions import vorticity_field  # noqa: E402


def kaplan_yorke(lam):
    """Kaplan-Yorke dimension of a descending spectrum (a lower bound of K when the K exponents do not reach a negative sum)."""
    total, j = 0.0, 0
    for j, v in enumerate(lam):
        if total + v < 0:
            return j + total / abs(v), True
        total += v
    return float(len(lam)), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--tangents", type=int, default=8, help="K: exponents to compute")
    ap.add_argument("--spinup", type=int, default=2000, help="steps of the plain fused solver before the measurement")
    ap.add_argument("--rounds", type=int, default=200, help="re-orthonormalisations")
    ap.add_argument("--inner", type=int, default=20, help="tangent steps between two re-orthonormalisations")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda:0")
    n, diam, K, B = args.n, 2 * math.pi, args.tangents, args.batch
    grid = tc.Grid(shape=(n, n), domain=((0, diam), (0, diam)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
    op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    dt = tc.stable_time_step(dx=diam / n, max_velocity=7.0, max_courant_number=0.5, viscosity=1e-3)
    plan = tc.fft_plan(n, torch.complex128, dev, diam=diam)
    w = plan.rfft2(vorticity_field(grid, 4, device=dev, batch_seeds=list(range(B))))
    with torch.no_grad():
        w, _ = op(w, dt, steps=args.spinup)          # onto the attractor
    dW = torch.stack([plan.rfft2(vorticity_field(grid, 8, device=dev, batch_seeds=[100 + 1000 * k + s for s in range(B)]))
                      for k in range(K)])
    dW, _ = tc.orthonormalize_tangents(dW, n)
    log_r = torch.zeros(B, K, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(1, args.rounds + 1):
        w, dW = op.tangent_bundle_step(w, dW, dt, steps=args.inner)
        dW, R = tc.orthonormalize_tangents(dW, n)
        log_r += torch.log(torch.diagonal(R, dim1=-2, dim2=-1))
        if r % max(1, args.rounds // 10) == 0:
            lam = (log_r / (r * args.inner * dt)).mean(0).cpu()
            print(f"t = {r * args.inner * dt:8.3f}   lambda_1..{K} (mean of {B} samples) = {[round(v, 3) for v in lam.tolist()]}")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    T = args.rounds * args.inner * dt
    lam = (log_r / T).cpu()
    mean, std = lam.mean(0), (lam.std(0) if B > 1 else torch.full((K,), float("nan")))
    print(f"Lyapunov spectrum after t = {T:.2f} ({B} samples, mean +- scatter):")
    for k in range(K):
        print(f"  lambda_{k + 1} = {mean[k].item():+.4f} +- {std[k].item():.4f}")
    dims = [kaplan_yorke(row.tolist()) for row in lam]
    closed = all(c for _, c in dims)
    d = torch.tensor([v for v, _ in dims])
    print(f"Kaplan-Yorke dimension: {d.mean().item():.2f} +- {d.std().item() if B > 1 else float('nan'):.2f}"
          + ("" if closed else f"  (a lower bound: the sum of the {K} exponents is still positive, raise --tangents)"))
    print(f"lambda_1 = {mean[0].item():.4f} +- {std[0].item():.4f}; examples/kolmogorov_lyapunov.py records 0.60 +- 0.12 for this flow")
    print(f"{args.rounds * args.inner} steps of {B} states with {K} tangents each and {args.rounds} QR factorisations took {wall:.2f} s "
          f"({wall / (args.rounds * args.inner) * 1e3:.3f} ms per step); state finite: {bool(torch.isfinite(torch.view_as_real(w)).all())}")


if __name__ == "__main__":
    main()
