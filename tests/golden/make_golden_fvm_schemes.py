#!/usr/bin/env python
"""Generate tests/golden/fvm_schemes_<scheme>.npz -- the finite-volume solver with each advection scheme -- by IMPORTING THE
REFERENCE (torch_cfd/fvm.py advect_general, interpolation.py linear / upwind / lax_wendroff / apply_tvd_limiter).  Run inside
the build container only:

    python tests/golden/make_golden_fvm_schemes.py

One file per scheme (all four in one file would pass the 1 MiB limit of a committed file).  The outputs hold inputs + the
reference's outputs, no reference source; nothing at test / bench time reads the reference.  Deterministic (seeded CPU
generators, CPU arithmetic): a rerun rewrites the files bit for bit.

Each file: n = 16, fp64, the A1 physics of fvm_edges.npz (nu = 1e-3, drag 0.1, Kolmogorov k = 2, dt = h / 4), for every
fvm_ops.EDGE_STARTS start and the smooth seed-0 start `smooth`:
    <start>_u0, <start>_cot, dt          inputs
    <start>_convect, <start>_explicit    the advection term alone and the explicit terms
    <start>_classic_rk4_1, _3            1 and 3 classic RK4 steps
    <start>_explicit_vjp, <start>_forward_euler_vjp    gradients of <cot, .> (smooth: classic_rk4_3_vjp as well)
and one fp32 group (n = 64, default dtype float32, the physics of fvm_small_f32.npz): f32_v0, f32_dt, f32_explicit,
f32_classic_rk4_1, f32_classic_rk4_10 (`linear` is not TVD: no run is longer than 10 steps).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))   # tests/: fvm_ops holds the degenerate starts and the cotangents the tests share

from torch_cfd import boundaries, grids, interpolation  # noqa: E402
from torch_cfd.equations import stable_time_step  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing  # noqa: E402
from torch_cfd.fvm import NavierStokes2DFVMProjection, RKStepper, advect_general  # noqa: E402
from torch_cfd.initial_conditions import filtered_velocity_field  # noqa: E402

import fvm_ops as F  # noqa: E402

L = 2 * np.pi
SCHEMES = {
    "upwind": lambda: interpolation.upwind,
    "linear": lambda: interpolation.linear,
    "lax_wendroff": lambda: interpolation.lax_wendroff,
    # built explicitly: the goldens of this scheme equal those of the reference's default convect
    "van_leer": lambda: interpolation.apply_tvd_limiter(interpolation.lax_wendroff, limiter=interpolation.van_leer_limiter),
}


def convect_of(c_interpolation_fn):
    def convect(v, dt):
        return grids.GridArrayVector(tuple(advect_general(u, v, interpolation.linear, c_interpolation_fn, dt) for u in v))
    return convect


def arr(v):
    return np.stack([c.data.detach().cpu().numpy() for c in v])


def build(n, nu, drag, wave, convect, stepper):
    grid = grids.Grid((n, n), domain=((0, L), (0, L)))
    bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)
    forcing = KolmogorovForcing(diam=L, wave_number=wave, grid=grid, offsets=((1.0, 0.5), (0.5, 1.0)))
    eq = NavierStokes2DFVMProjection(viscosity=nu, grid=grid, bcs=(bc, bc), density=1.0, drag=drag, convect=convect,
                                     forcing=forcing, solver=stepper)
    return grid, eq


def named(method):
    return RKStepper.from_method(method=method, requires_grad=False, dtype=torch.float32)


def run(v, stepper, eq, dt, steps):
    with torch.no_grad():
        for _ in range(steps):
            v = stepper.forward(v, dt, equation=eq)
    return v


def rollout(stepper, eq, dt, k):
    def fn(v):
        for _ in range(k):
            v = stepper.forward(v, dt, equation=eq)
        return v
    return fn


def state_of(arrays, like, leaves=False):
    vs = [grids.GridVariable(grids.GridArray(a.clone().requires_grad_(leaves), c.offset, c.grid), c.bc)
          for a, c in zip(arrays, like)]
    return grids.GridVariableVector(vs), [v.data for v in vs]


def vjp(fn, arrays, like, cot):
    """Gradient of sum(cot * fn(state)) with respect to the two velocity arrays."""
    v, leaves = state_of(arrays, like, leaves=True)
    out = fn(v)
    loss = sum((c.data * g).sum() for c, g in zip(out, cot))
    return np.stack([g.numpy() for g in torch.autograd.grad(loss, leaves)])


def scheme_file(name):
    n, wave, nu, drag = 16, 2, 1e-3, 0.1
    convect = convect_of(SCHEMES[name]())
    rk4, euler = named("classic_rk4"), named("forward_euler")
    grid, eq = build(n, nu, drag, wave, convect, rk4)
    like = filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=0)
    dt = 0.25 * min(grid.step)
    starts = list(F.EDGE_STARTS) + ["smooth"]
    out = {"n": n, "wave": wave, "nu": nu, "drag": drag, "dt": dt, "starts": np.array(starts), "scheme": np.array(name)}
    for si, start in enumerate(starts):
        if start == "smooth":
            u = torch.stack([c.data.detach() for c in like])
        else:
            u = F.degenerate_start(start, n, seed=100 + si)   # the starts of fvm_edges.npz
        cot = F.cotangent((2, n, n), 500 + si)
        v, _ = state_of(u, like)
        out[f"{start}_u0"], out[f"{start}_cot"] = u.numpy(), cot.numpy()
        with torch.no_grad():
            out[f"{start}_convect"] = arr(convect(v, dt))
            out[f"{start}_explicit"] = arr(eq.explicit_terms(v, dt))
            out[f"{start}_classic_rk4_1"] = arr(run(v, rk4, eq, dt, 1))
            out[f"{start}_classic_rk4_3"] = arr(run(v, rk4, eq, dt, 3))
        out[f"{start}_explicit_vjp"] = vjp(lambda w: eq.explicit_terms(w, dt), u, like, cot)
        out[f"{start}_forward_euler_vjp"] = vjp(rollout(euler, eq, dt, 1), u, like, cot)
        if start == "smooth":
            out[f"{start}_classic_rk4_3_vjp"] = vjp(rollout(rk4, eq, dt, 3), u, like, cot)

    # fp32 fields (default dtype float32 throughout, as a float32 run of the reference): small() of make_golden_fvm.py
    n32, nu32, drag32, wave32 = 64, 1e-3, 0.1, 4
    dt32 = stable_time_step(dx=L / n32, max_velocity=2.0, max_courant_number=0.5, viscosity=nu32)
    torch.set_default_dtype(torch.float32)
    grid, eq = build(n32, nu32, drag32, wave32, convect, rk4)
    v32 = filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=42)
    out["f32_n"], out["f32_wave"], out["f32_dt"], out["f32_v0"] = n32, wave32, dt32, arr(v32)
    with torch.no_grad():
        out["f32_explicit"] = arr(eq.explicit_terms(v32, dt32))
    out["f32_classic_rk4_1"] = arr(run(v32, rk4, eq, dt32, 1))
    out["f32_classic_rk4_10"] = arr(run(v32, rk4, eq, dt32, 10))
    torch.set_default_dtype(torch.float64)
    assert out["f32_explicit"].dtype == np.float32

    for k, v in out.items():
        a = np.asarray(v)
        assert a.dtype.kind in "US" or np.isfinite(a).all(), (name, k)
    path = os.path.join(HERE, f"fvm_schemes_{name}.npz")
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name in SCHEMES:
        path = scheme_file(name)
        print(os.path.basename(path), os.path.getsize(path))
