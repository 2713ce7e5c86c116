#!/usr/bin/env python
"""Generate tests/golden/ns2d_ensemble.npz -- ensembles with per-sample viscosity, drag and forcing amplitude -- by IMPORTING
THE REFERENCE (torch_cfd/equations.py, forcings.py, initial_conditions.py) and running it on the CPU.  Run inside the build
container only:

    python tests/golden/make_golden_ns2d_ensemble.py

Every stored result is B SCALAR reference runs stacked (member b: viscosity NU[b], drag DRAG[b], Kolmogorov forcing of amplitude
FSCALE[b]); the reference's own broadcast form -- ``viscosity=tensor(NU).view(B, 1, 1)``, ``drag=tensor(DRAG).view(B, 1, 1)`` --
is asserted to agree with them to 1e-12 in fp64 (for the members it can express: it has no per-sample forcing amplitude, so
with the amplitudes all 1).  The file holds inputs and the reference's results, no reference source; nothing at test time reads
the reference.  Deterministic (seeded CPU generators, CPU arithmetic).

Keys (n = 64, B = 4; ``f64_`` complex128, ``f32_`` complex64): ``w0`` (f64 only: the complex64 run starts from its rounding,
asserted here), ``F``, ``w1``, ``w10`` (RK4-CN, 1 / 10 steps of dt), ``res1`` (residual of (w1, dwdt1)), ``imex2`` (one
IMEXStepper(order=2) step); ``g32_w0`` / ``{tag}_g32_grad``: at n = 32, the gradient of sum |w3|^2 (3 RK4-CN steps) with respect
to w0.  dwdt1 / dwdt10 are NOT stored: the reference forms them as ``1 / (steps * dt) * (w_new - w0)``, one rounded subtraction and
one rounded product per component, which this script asserts bit for bit -- the tests form them from the stored states by the
same two operations (and the file stays within the size limit of a committed file).
"""
import io
import math
import os
import sys
import zipfile

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
N, NG, B, DT = 64, 32, 4, 1e-3
NU = (1e-3, 1e-2, 5e-2, 2e-1)
DRAG = (0.1, 0.0, 0.5, 0.05)
FSCALE = (1.0, 0.0, -2.0, 0.5)
CPLX = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def rel_l2(a, b):
    a, b = (torch.as_tensor(x).to(torch.complex128) for x in (a, b))
    return (torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1))).item()


def scalar_op(grid, nu, drag, fscale, solver):
    forcing = KolmogorovForcing(grid=grid, scale=fscale, wave_number=4, swap_xy=False)
    return NavierStokes2DSpectral(viscosity=nu, grid=grid, drag=drag, smooth=True, forcing_fn=forcing, solver=solver)


def stacked(grid, w0, fn, solver=RK4CrankNicolsonStepper, nu=NU, drag=DRAG, fscale=FSCALE):
    """fn(op, w) of member b's scalar reference operator on w0[b:b+1], stacked over b."""
    outs = [fn(scalar_op(grid, nu[b], drag[b], fscale[b], solver()), w0[b:b + 1]) for b in range(B)]
    return torch.cat(outs)


def initial(grid, real):
    torch.set_default_dtype(torch.float64)
    w = torch.fft.rfft2(torch.stack([vorticity_field(grid, 4, s).data for s in range(B)]))
    torch.set_default_dtype(real)
    return w.to(CPLX[real])


def run(out, real, tag):
    torch.set_default_dtype(real)
    grid = Grid(shape=(N, N), domain=((0, L), (0, L)))
    w0 = initial(grid, real)
    if real == torch.float64:
        out["f64_w0"] = w0.numpy()
    else:
        assert np.array_equal(w0.numpy(), out["f64_w0"].astype(np.complex64))   # the tests start the fp32 run from this rounding
    res = {}
    res["F"] = stacked(grid, w0, lambda op, w: op.explicit_terms(w))
    res["w1"] = stacked(grid, w0, lambda op, w: op(w, DT)[0])
    d1 = stacked(grid, w0, lambda op, w: op(w, DT)[1])
    res["w10"] = stacked(grid, w0, lambda op, w: op(w, DT, steps=10)[0])
    d10 = stacked(grid, w0, lambda op, w: op(w, DT, steps=10)[1])
    # dw/dt is not stored: 1 / (steps dt) * (w_new - w0), bit for bit
    assert torch.equal(d1, 1 / (1 * DT) * (res["w1"] - w0)) and torch.equal(d10, 1 / (10 * DT) * (res["w10"] - w0))

    def residual(op, w):
        w1, dw1 = op(w, DT)
        return op.residual(w1, dw1)

    res["res1"] = stacked(grid, w0, residual)
    res["imex2"] = stacked(grid, w0, lambda op, w: op(w, DT)[0], solver=lambda: IMEXStepper(order=2))
    for k, v in res.items():
        out[f"{tag}_{k}"] = v.numpy()

    # (1) the reference's own broadcast form against the stacked scalar runs (forcing amplitudes 1: it has no per-sample amplitude)
    ones = (1.0,) * B
    bop = NavierStokes2DSpectral(viscosity=torch.tensor(NU, dtype=real).view(B, 1, 1), grid=grid,
                                 drag=torch.tensor(DRAG, dtype=real).view(B, 1, 1), smooth=True,
                                 forcing_fn=KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False),
                                 solver=RK4CrankNicolsonStepper())
    ref10 = stacked(grid, w0, lambda op, w: op(w, DT, steps=10)[0], fscale=ones)
    err = rel_l2(bop(w0, DT, steps=10)[0], ref10)
    print(f"{tag}: reference broadcast form vs stacked scalar runs, 10 steps: {err:.3e}")
    if real == torch.float64:
        assert err < 1e-12, err

    # (2) every single parameter of a member matters: a member stepped with a neighbour's value cannot pass
    for name, values in (("nu", NU), ("drag", DRAG), ("fscale", FSCALE)):
        worst = math.inf
        for b in range(B):
            other = values[(b + 1) % B]
            kw = {"nu": NU[b], "drag": DRAG[b], "fscale": FSCALE[b]}
            kw[name] = other
            op = scalar_op(grid, kw["nu"], kw["drag"], kw["fscale"], RK4CrankNicolsonStepper())
            worst = min(worst, rel_l2(op(w0[b:b + 1], DT, steps=10)[0], res["w10"][b:b + 1]))
        print(f"{tag}: {name} of a neighbour moves w10 by at least {worst:.3e}")
        assert worst > 1e-4, (name, worst)

    # gradient of sum |w3|^2 with respect to w0, n = 32
    gridg = Grid(shape=(NG, NG), domain=((0, L), (0, L)))
    torch.set_default_dtype(torch.float64)
    wg = torch.fft.rfft2(torch.stack([vorticity_field(gridg, 4, 100 + s).data for s in range(B)]))
    torch.set_default_dtype(real)
    if real == torch.float64:
        out["g32_w0"] = wg.numpy()
    wg = wg.to(CPLX[real])

    def grad(op, w):
        w = w.clone().requires_grad_(True)
        w3, _ = op(w, DT, steps=3)
        (w3.abs() ** 2).sum().backward()
        return w.grad

    out[f"{tag}_g32_grad"] = stacked(gridg, wg, grad).numpy()


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"dt": DT, "nu": np.array(NU), "drag": np.array(DRAG), "fscale": np.array(FSCALE)}
    run(out, torch.float64, "f64")
    run(out, torch.float32, "f32")
    torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "ns2d_ensemble.npz")
    # an .npz is a zip of .npy members, and numpy reads whatever method the zip names: LZMA brings these (mostly incompressible)
    # spectra 3 % further down than np.savez_compressed's deflate -- under the size limit of a committed file
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as z:
        for k, v in out.items():
            buf = io.BytesIO()
            np.save(buf, np.asarray(v))
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_LZMA)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20
    for k, v in out.items():
        a = np.asarray(v)
        if a.ndim >= 3:
            print(f"{k:16s} {a.dtype} {a.shape} finite={np.isfinite(a).all()} max={np.abs(a).max():.3e}")
