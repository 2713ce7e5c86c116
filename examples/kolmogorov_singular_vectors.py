#!/usr/bin/env python
"""The K leading singular values and right singular vectors of the propagator of Kolmogorov-forced 2-D turbulence over a window:
block subspace iteration on J^T J with the tangent bundle and the cotangent bundle.

J is the Jacobian of ``steps`` steps of the solver at a state on the attractor.  Each iteration applies it to a block V of
orthonormal perturbations with ``tangent_bundle_step`` (U = J V), applies its transpose with ``adjoint_bundle_step``
(Z = J^T U) -- the state's share of every stage done once per call for the whole block -- and re-orthonormalises Z with
``orthonormalize_tangents``; a Rayleigh-Ritz step on the small matrix <U_i, U_j> turns the block into singular-vector
estimates.  The block carries a few guard vectors beyond the K that are reported, which is what sets the convergence rate
(sigma_{K + guard + 1} / sigma_k)^2 per iteration.

Everything is measured in the real-field inner product <a, b> = sum_x a(x) b(x).  The library's transpose is taken in the
plain product of the half spectra, sum Re(conj(a^) b^); with the column weights c of ``real_field_weights`` the adjoint in the
real-field product is  J* = c^-1 J^T c,  applied to the part of a half spectrum that a real field produces (the ky = 0 and
Nyquist columns made Hermitian in kx -- what irfft2 sees of them).  Same flow as examples/kolmogorov_lyapunov.py: fp64,
Kolmogorov forcing k = 4, drag 0.1, nu = 1e-3, on generated data.

    python examples/kolmogorov_singular_vectors.py [--n 128] [--k 4] [--guard 4] [--steps 50] [--spinup 1000] [--iterations 60] [--tol 1e-8]

It prints sigma_k and the relative residual |J*J v_k - sigma_k^2 v_k| / sigma_k^2 of every reported pair.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd.spectral import real_field_weights  # noqa: E402


def visible(A, n):
    """The part of the half spectra ``A`` (..., n, m) that a real field produces: columns ky = 0 and (even n) Nyquist made
    Hermitian in kx.  An orthogonal projection in the real-field inner product."""
    own = [0] + ([A.shape[-1] - 1] if n % 2 == 0 else [])
    cols = A[..., own]
    out = A.clone()
    out[..., own] = 0.5 * (cols + torch.roll(cols.flip(-2), 1, -2).conj())
    return out


def singular_vectors(apply_j, apply_jt, V, n, keep, iterations, tol, log=print):
    """Block subspace iteration on J*J.  ``apply_j(V)`` / ``apply_jt(G)`` map a block (K, n, m) of half spectra through J and
    through its transpose in the plain half-spectrum product.  Returns ``(sigma, V, residual)`` for the ``keep`` leading pairs."""
    c = real_field_weights(n, V.shape[-1], V.real.dtype, V.device)
    inner = lambda A, B: torch.einsum("ixy,jxy,y->ij", A.real, B.real, c) + torch.einsum("ixy,jxy,y->ij", A.imag, B.imag, c)
    V, _ = tc.orthonormalize_tangents(visible(V, n), n)
    for it in range(1, iterations + 1):
        U = visible(apply_j(V), n)                        # J V
        Z = visible(apply_jt(U * c) / c, n)               # J* J V
        theta, Y = torch.linalg.eigh(inner(U, U))         # Rayleigh-Ritz on <V_i, J*J V_j> = <U_i, U_j>
        theta, Y = theta.flip(0), Y.flip(1).to(V.dtype)
        Vr, Zr = torch.einsum("kxy,kj->jxy", V, Y), torch.einsum("kxy,kj->jxy", Z, Y)
        R = Zr - theta[:, None, None] * Vr
        res = torch.sqrt(torch.diagonal(inner(R, R))) / theta
        sigma = torch.sqrt(theta)
        log(f"iteration {it:3d}: sigma_1..{keep} = {[round(v, 6) for v in sigma[:keep].tolist()]}  largest residual {res[:keep].max().item():.2e}")
        if res[:keep].max().item() <= tol:
            break
        V, _ = tc.orthonormalize_tangents(Z, n)
    return sigma[:keep], Vr[:keep], res[:keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--k", type=int, default=4, help="K: singular pairs to report")
    ap.add_argument("--guard", type=int, default=4, help="further vectors the block carries (they set the convergence rate)")
    ap.add_argument("--steps", type=int, default=50, help="steps of the window")
    ap.add_argument("--spinup", type=int, default=1000, help="steps of the plain fused solver before the window")
    ap.add_argument("--iterations", type=int, default=60, help="at most this many applications of J*J")
    ap.add_argument("--tol", type=float, default=1e-8, help="stop when every reported relative residual is below this")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda:0")
    n, diam, K = args.n, 2 * math.pi, args.k + args.guard
    grid = tc.Grid(shape=(n, n), domain=((0, diam), (0, diam)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
    op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    dt = tc.stable_time_step(dx=diam / n, max_velocity=7.0, max_courant_number=0.5, viscosity=1e-3)
    plan = tc.fft_plan(n, torch.complex128, dev, diam=diam)
    from torch_cfd_amd.initial_conditions import vorticity_field

    w = plan.rfft2(vorticity_field(grid, 4, device=dev, batch_seeds=[0]))[0]
    with torch.no_grad():
        w, _ = op(w, dt, steps=args.spinup)          # onto the attractor
    V = plan.rfft2(vorticity_field(grid, 8, device=dev, batch_seeds=[100 + s for s in range(K)]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sigma, Vk, res = singular_vectors(lambda X: op.tangent_bundle_step(w, X, dt, steps=args.steps)[1],
                                      lambda G: op.adjoint_bundle_step(w, G, dt, steps=args.steps)[1], V, n, args.k,
                                      args.iterations, args.tol)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"leading singular values of the propagator over t = {args.steps * dt:.3f} ({args.steps} steps, {n} x {n}):")
    for k in range(args.k):
        print(f"  sigma {sigma[k].item():.10f}   residual {res[k].item():.3e}")
    print(f"{wall:.2f} s; vectors finite: {bool(torch.isfinite(torch.view_as_real(Vk)).all())}")


if __name__ == "__main__":
    main()
