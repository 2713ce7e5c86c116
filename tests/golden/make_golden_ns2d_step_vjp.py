#!/usr/bin/env python
"""Generate tests/golden/ns2d_step_vjp.npz -- reverse-mode gradients through whole steps of the spectral solver -- by IMPORTING
THE REFERENCE (torch_cfd/equations.py, forcings.py, initial_conditions.py) and calling torch.autograd on it (its step is plain
torch ops).  Run inside the build container only:

    python tests/golden/make_golden_ns2d_step_vjp.py

The file holds inputs, fixed cotangents and the reference's gradients, no reference source; nothing at test time reads the
reference.  Deterministic (seeded CPU generators, CPU arithmetic): a rerun rewrites the file bit for bit.

Keys: ``w0`` / ``cot`` (B, n, m) complex128 state and cotangent of the stepped state; ``{forcing}_s{smooth}_{what}`` =
``w.grad`` of ``sum Re(conj(cot) . forward(w, dt)^K)`` with what = ``rk1`` / ``rk3`` (RK4-CN, K = 1 / 3), ``imex1`` /
``imex1.5`` / ``imex2`` (IMEXStepper orders, K = 2; order 2 restarts its second stage from the step's initial state);
``f32_*``: the same quantities of one complex64 run.
"""
import math
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

from torch_cfd.equations import IMEXStepper, NavierStokes2DSpectral, RK4CrankNicolsonStepper  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing  # noqa: E402
from torch_cfd.grids import Grid  # noqa: E402
from torch_cfd.initial_conditions import vorticity_field  # noqa: E402

L = 2 * math.pi
N, B, DT, NU = 16, 2, 1e-3, 1e-3
FORCINGS = {"none": 0.0, "kolmogorov": 0.1}   # name -> drag
IMEX = ((1, 1.0, 1.0), (1.5, 0.5, 0.5), (2, 0.5, 0.5))       # order, alpha, beta


def make_op(grid, forcing, smooth, solver):
    fn = KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False) if forcing == "kolmogorov" else None
    return NavierStokes2DSpectral(viscosity=NU, grid=grid, drag=FORCINGS[forcing], smooth=smooth, forcing_fn=fn, solver=solver)


def gradient(op, w0, cot, steps):
    w = w0.clone().requires_grad_(True)
    out = w
    for _ in range(steps):
        out = op(out, DT, steps=1)[0]
    (out.real * cot.real + out.imag * cot.imag).sum().backward()
    return w.grad.detach().numpy()


def inputs(grid, real):
    torch.set_default_dtype(real)
    w0 = torch.fft.rfft2(torch.stack([vorticity_field(grid, 4, s).data for s in range(B)]))
    gen = torch.Generator().manual_seed(4321)
    cot = torch.view_as_complex(torch.randn(B, N, N // 2 + 1, 2, generator=gen, dtype=torch.float64).to(real))
    return w0, cot


def cases(out, real, combos, prefix=""):
    torch.set_default_dtype(real)
    grid = Grid(shape=(N, N), domain=((0, L), (0, L)))
    w0, cot = inputs(grid, real)
    out[prefix + "w0"], out[prefix + "cot"] = w0.numpy(), cot.numpy()
    for forcing, smooth in combos:
        key = f"{prefix}{forcing}_s{int(smooth)}_"
        op = make_op(grid, forcing, smooth, RK4CrankNicolsonStepper())
        out[key + "rk1"] = gradient(op, w0, cot, 1)
        out[key + "rk3"] = gradient(op, w0, cot, 3)
        for order, alpha, beta in IMEX:
            op = make_op(grid, forcing, smooth, IMEXStepper(order=order, alpha=alpha, beta=beta))
            out[key + f"imex{order}"] = gradient(op, w0, cot, 2)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"dt": DT, "nu": NU}
    cases(out, torch.float64, [(f, s) for f in FORCINGS for s in (True, False)])
    cases(out, torch.float32, [("kolmogorov", True)], prefix="f32_")
    torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "ns2d_step_vjp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k, v in out.items():
        a = np.asarray(v)
        if a.ndim >= 3:
            print(f"{k:28s} {a.dtype} {a.shape} finite={np.isfinite(a).all()} max={np.abs(a).max():.3e}")
