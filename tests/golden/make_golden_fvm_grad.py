#!/usr/bin/env python
"""Generate tests/golden/fvm_grad.npz -- gradients of the finite-volume solver -- by IMPORTING THE REFERENCE
(torch_cfd/fvm.py, pressure.py, forcings.py, initial_conditions.py) and running torch autograd through it.  Run inside the
build container only:

    python tests/golden/make_golden_fvm_grad.py

The file holds inputs, fixed cotangents and the reference's gradients, no reference source; nothing at test time reads
the reference.  A batch of B samples is B independent reference runs stacked (the samples do not interact).
Deterministic (seeded CPU generators, CPU arithmetic): a rerun rewrites the file bit for bit.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from torch_cfd import boundaries, grids  # noqa: E402
from torch_cfd.equations import stable_time_step  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing  # noqa: E402
from torch_cfd.fvm import NavierStokes2DFVMProjection, RKStepper  # noqa: E402
from torch_cfd.initial_conditions import filtered_velocity_field  # noqa: E402

L = 2 * np.pi
METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")
NU, DRAG, WAVE, VMAX = 1e-3, 0.1, 4, 2.0


def grid_of(n):
    return grids.Grid((n, n), domain=((0, L), (0, L)))


def equation(n, method):
    grid = grid_of(n)
    forcing = KolmogorovForcing(diam=L, wave_number=WAVE, grid=grid, offsets=((1.0, 0.5), (0.5, 1.0)))
    bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)
    stepper = RKStepper.from_method(method=method, requires_grad=False, dtype=torch.float32)
    return NavierStokes2DFVMProjection(viscosity=NU, grid=grid, bcs=(bc, bc), density=1.0, drag=DRAG, forcing=forcing,
                                       solver=stepper), stepper


def leaf_state(arrays, like):
    """GridVariableVector whose arrays are fresh leaves that require grad (offsets and bcs of `like`)."""
    vs = [grids.GridVariable(grids.GridArray(a.clone().requires_grad_(), c.offset, c.grid), c.bc)
          for a, c in zip(arrays, like)]
    return grids.GridVariableVector(vs), [v.data for v in vs]


def vjp(fn, arrays, like, cot):
    """Gradient of sum(cot * fn(state)) with respect to the two velocity arrays."""
    v, leaves = leaf_state(arrays, like)
    out = fn(v)
    loss = sum((c.data * g).sum() for c, g in zip(out, cot))
    return np.stack([g.numpy() for g in torch.autograd.grad(loss, leaves)])


def initial(n, seed, dtype):
    v = filtered_velocity_field(grid_of(n), VMAX, 3.0, iterations=3, random_state=seed)
    return [c.data.detach().to(dtype) for c in v], v


def cotangent(n, batch, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 2, n, n, generator=gen, dtype=torch.float64).to(dtype)


def terms(out):
    """explicit-terms and projection VJPs at n = 32, fp64."""
    n = 32
    grid = grid_of(n)
    dt = stable_time_step(dx=min(grid.step), max_velocity=VMAX, max_courant_number=0.5, viscosity=NU)
    arrays, like = initial(n, 11, torch.float64)
    eq, _ = equation(n, "classic_rk4")
    cot = cotangent(n, 1, 101, torch.float64)[0]
    out["terms_dt"] = dt
    out["terms_u"] = np.stack([a.numpy() for a in arrays])
    out["terms_cot"] = cot.numpy()
    out["terms_explicit_vjp"] = vjp(lambda v: eq.explicit_terms(v, dt), arrays, like, cot)
    gen = torch.Generator().manual_seed(102)
    raw = [torch.randn(n, n, generator=gen, dtype=torch.float64) for _ in range(2)]
    out["proj_u"] = np.stack([a.numpy() for a in raw])
    out["proj_vjp"] = vjp(lambda v: eq.pressure_projection(v), raw, like, cot)


def steps(out, n, batch, dtype=torch.float64, methods=METHODS, counts=(1, 3), tag=None):
    """`counts` steps of each method from `batch` seeded initial conditions, Kolmogorov forcing k = 4, drag 0.1."""
    tag = tag or f"n{n}_b{batch}"
    grid = grid_of(n)
    dt = stable_time_step(dx=min(grid.step), max_velocity=VMAX, max_courant_number=0.5, viscosity=NU)
    states = [initial(n, 20 + s, dtype) for s in range(batch)]
    cot = cotangent(n, batch, 200 + n + batch, dtype)
    out[f"{tag}_dt"] = dt
    out[f"{tag}_u0"] = np.stack([np.stack([a.numpy() for a in arrays]) for arrays, _ in states])
    out[f"{tag}_cot"] = cot.numpy()
    for m in methods:
        eq, stepper = equation(n, m)
        for k in counts:
            def run(v, k=k):
                for _ in range(k):
                    v = stepper.forward(v, dt, equation=eq)
                return v
            out[f"{tag}_{m}_{k}"] = np.stack([vjp(run, arrays, like, cot[s]) for s, (arrays, like) in enumerate(states)])


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"nu": NU, "drag": DRAG, "wave": WAVE}
    terms(out)
    steps(out, 16, 2)
    steps(out, 32, 1)
    # fp32 fields (default dtype float32 throughout, as a float32 run of the reference)
    torch.set_default_dtype(torch.float32)
    steps(out, 32, 1, torch.float32, methods=("classic_rk4",), counts=(3,), tag="f32")
    torch.set_default_dtype(torch.float64)
    path = os.path.join(HERE, "fvm_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k, v in out.items():
        a = np.asarray(v)
        if a.ndim >= 3:
            print(f"{k:32s} {a.dtype} {a.shape} finite={np.isfinite(a).all()} max={np.abs(a).max():.3e}")
