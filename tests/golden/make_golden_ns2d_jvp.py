#!/usr/bin/env python
"""Generate tests/golden/ns2d_jvp.npz -- forward-mode tangents of the spectral solver -- by IMPORTING THE REFERENCE
(torch_cfd/equations.py, forcings.py, initial_conditions.py) and running torch.autograd.forward_ad through it (its step is
plain torch ops).  Run inside the build container only:

    python tests/golden/make_golden_ns2d_jvp.py

The file holds inputs, fixed perturbations and the reference's tangents, no reference source; nothing at test time reads the
reference.  Deterministic (seeded CPU generators, CPU arithmetic): a rerun rewrites the file bit for bit.

Keys: ``w0`` / ``dw`` (B, n, m) complex128 state and perturbation (the perturbation is the half spectrum of a real field);
``{forcing}_s{smooth}_{what}`` with what = ``F`` (tangent of the explicit terms), ``rk1`` / ``rk3`` (RK4-CN, 1 / 3 steps),
``imex1`` / ``imex1.5`` / ``imex2`` (IMEXStepper orders, 2 steps); ``f32_*``: the same quantities of one complex64 run.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

from torch_cfd.equations import IMEXStepper, NavierStokes2DSpectral, RK4CrankNicolsonStepper  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing, SinCosForcing  # noqa: E402
from torch_cfd.grids import Grid  # noqa: E402
from torch_cfd.initial_conditions import vorticity_field  # noqa: E402

L = 2 * math.pi
N, B, DT, NU = 16, 2, 1e-3, 1e-3
FORCINGS = {"none": 0.0, "kolmogorov": 0.1, "sincos": 0.0}   # name -> drag
IMEX = ((1, 1.0, 1.0), (1.5, 0.5, 0.5), (2, 0.5, 0.5))       # order, alpha, beta


def make_op(grid, forcing, smooth, solver):
    if forcing == "kolmogorov":
        fn = KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False)
    elif forcing == "sincos":
        fn = SinCosForcing(grid=grid, scale=0.1, k=1.0, diam=L)
    else:
        fn = None
    return NavierStokes2DSpectral(viscosity=NU, grid=grid, drag=FORCINGS[forcing], smooth=smooth, forcing_fn=fn, solver=solver)


def tangent(fn, w, dw):
    with fwAD.dual_level():
        out = fn(fwAD.make_dual(w, dw))
        out = out[0] if isinstance(out, tuple) else out
        return fwAD.unpack_dual(out).tangent.detach().numpy()


def inputs(grid, real):
    torch.set_default_dtype(real)
    w0 = torch.fft.rfft2(torch.stack([vorticity_field(grid, 4, s).data for s in range(B)]))
    gen = torch.Generator().manual_seed(1234)
    dw = torch.fft.rfft2(torch.randn(B, N, N, generator=gen, dtype=torch.float64).to(real))
    return w0, dw


def cases(out, real, combos, prefix=""):
    torch.set_default_dtype(real)
    grid = Grid(shape=(N, N), domain=((0, L), (0, L)))
    w0, dw = inputs(grid, real)
    out[prefix + "w0"], out[prefix + "dw"] = w0.numpy(), dw.numpy()
    for forcing, smooth in combos:
        key = f"{prefix}{forcing}_s{int(smooth)}_"
        op = make_op(grid, forcing, smooth, RK4CrankNicolsonStepper())
        out[key + "F"] = tangent(op.explicit_terms, w0, dw)
        out[key + "rk1"] = tangent(lambda w: op(w, DT, steps=1), w0, dw)
        out[key + "rk3"] = tangent(lambda w: op(w, DT, steps=3), w0, dw)
        for order, alpha, beta in IMEX:
            op = make_op(grid, forcing, smooth, IMEXStepper(order=order, alpha=alpha, beta=beta))
            out[key + f"imex{order}"] = tangent(lambda w: op(w, DT, steps=2), w0, dw)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"dt": DT, "nu": NU}
    cases(out, torch.float64, [(f, s) for f in FORCINGS for s in (True, False)])
    cases(out, torch.float32, [("kolmogorov", True)], prefix="f32_")
    torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "ns2d_jvp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k, v in out.items():
        a = np.asarray(v)
        if a.ndim >= 3:
            print(f"{k:28s} {a.dtype} {a.shape} finite={np.isfinite(a).all()} max={np.abs(a).max():.3e}")
