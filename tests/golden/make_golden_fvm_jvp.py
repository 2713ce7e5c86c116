#!/usr/bin/env python
"""Generate tests/golden/fvm_jvp.npz -- tangents (Jacobian-vector products) of the finite-volume solver -- by IMPORTING THE
REFERENCE (torch_cfd/fvm.py, pressure.py, interpolation.py, forcings.py) and running torch.autograd.forward_ad through it.
Run inside the build container only:

    python tests/golden/make_golden_fvm_jvp.py

To stay small the file holds no states: every state is one already in fvm_grad.npz (terms_u, proj_u, n16_b2_u0, n32_b1_u0,
f32_u0 and their dt) or in fvm_edges.npz (the a1_* degenerate starts).  It holds the seeded perturbations (`*_du`) and the
reference's tangents, floating-point arrays only, no reference source; nothing at test time reads the reference.  A batch of B
samples is B independent reference runs stacked.  Deterministic (seeded CPU generators, CPU arithmetic).

    terms_du, terms_explicit_jvp; proj_du, proj_jvp                         n = 32, physics of fvm_grad.npz
    <case>_du, <case>_<method>_<k>        case n16_b2 / n32_b1, the four named methods, k = 1 and 3 steps
    scheme_<scheme>_classic_rk4_3         3 classic RK4 steps of each advection scheme from n16_b2_u0 along n16_b2_du
    a1_<start>_du, a1_<start>_explicit_jvp, a1_<start>_forward_euler_jvp    the degenerate starts, physics A1 of fvm_edges.npz
    f32_du, f32_classic_rk4_3             default dtype float32 throughout, as a float32 run of the reference
"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))   # tests/: fvm_ops names the degenerate starts

from torch_cfd import boundaries, grids, interpolation  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing  # noqa: E402
from torch_cfd.fvm import NavierStokes2DFVMProjection, RKStepper, advect_general  # noqa: E402
from torch_cfd.initial_conditions import filtered_velocity_field  # noqa: E402

import fvm_ops as F  # noqa: E402

L = 2 * np.pi
METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")
SCHEMES = {
    "upwind": lambda: interpolation.upwind,
    "linear": lambda: interpolation.linear,
    "lax_wendroff": lambda: interpolation.lax_wendroff,
    "van_leer": lambda: interpolation.apply_tvd_limiter(interpolation.lax_wendroff, limiter=interpolation.van_leer_limiter),
}


def grid_of(n):
    return grids.Grid((n, n), domain=((0, L), (0, L)))


def equation(n, method, nu, drag, wave, scheme=None):
    grid = grid_of(n)
    forcing = KolmogorovForcing(diam=L, wave_number=wave, grid=grid, offsets=((1.0, 0.5), (0.5, 1.0)))
    bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)
    stepper = RKStepper.from_method(method=method, requires_grad=False, dtype=torch.float32)
    kw = {}
    if scheme is not None:
        c_fn = SCHEMES[scheme]()
        kw["convect"] = lambda v, dt: grids.GridArrayVector(
            tuple(advect_general(u, v, interpolation.linear, c_fn, dt) for u in v))
    return NavierStokes2DFVMProjection(viscosity=nu, grid=grid, bcs=(bc, bc), density=1.0, drag=drag, forcing=forcing,
                                       solver=stepper, **kw), stepper


def like_of(n):
    """A velocity of the reference, for the offsets and boundary conditions of its components."""
    return filtered_velocity_field(grid_of(n), 2.0, 3.0, iterations=3, random_state=0)


def jvp(fn, u, du, like):
    """Tangent of fn(state) along du: (2, n, n) arrays in, (2, n, n) out, by dual numbers through the reference."""
    u, du = torch.as_tensor(u), torch.as_tensor(du)
    with fwAD.dual_level():
        vs = [grids.GridVariable(grids.GridArray(fwAD.make_dual(a.clone(), d.clone()), c.offset, c.grid), c.bc)
              for a, d, c in zip(u, du, like)]
        out = fn(grids.GridVariableVector(vs))
        tangents = [fwAD.unpack_dual(c.data).tangent for c in out]
        assert all(t is not None for t in tangents)
        return np.stack([t.detach().numpy() for t in tangents])


def perturbation(shape, seed, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype).numpy()


def rollout(stepper, eq, dt, k):
    def fn(v):
        for _ in range(k):
            v = stepper.forward(v, dt, equation=eq)
        return v
    return fn


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    grad = np.load(os.path.join(HERE, "fvm_grad.npz"))
    edges = np.load(os.path.join(HERE, "fvm_edges.npz"))
    nu, drag, wave = float(grad["nu"]), float(grad["drag"]), int(grad["wave"])
    out = {}

    # explicit terms and projection, n = 32
    eq, _ = equation(32, "classic_rk4", nu, drag, wave)
    like = like_of(32)
    dt = float(grad["terms_dt"])
    out["terms_du"] = perturbation((2, 32, 32), 301)
    out["terms_explicit_jvp"] = jvp(lambda v: eq.explicit_terms(v, dt), grad["terms_u"], out["terms_du"], like)
    out["proj_du"] = perturbation((2, 32, 32), 302)
    out["proj_jvp"] = jvp(lambda v: eq.pressure_projection(v), grad["proj_u"], out["proj_du"], like)

    # 1 and 3 steps of the named methods
    for case, n, batch in (("n16_b2", 16, 2), ("n32_b1", 32, 1)):
        u0, dt, like = grad[f"{case}_u0"], float(grad[f"{case}_dt"]), like_of(n)
        du = out[f"{case}_du"] = perturbation((batch, 2, n, n), 310 + n + batch)
        for m in METHODS:
            eq, stepper = equation(n, m, nu, drag, wave)
            for k in (1, 3):
                out[f"{case}_{m}_{k}"] = np.stack([jvp(rollout(stepper, eq, dt, k), u0[s], du[s], like) for s in range(batch)])

    # each advection scheme, 3 classic RK4 steps at n = 16
    u0, du, dt, like = grad["n16_b2_u0"], out["n16_b2_du"], float(grad["n16_b2_dt"]), like_of(16)
    for name in SCHEMES:
        eq, stepper = equation(16, "classic_rk4", nu, drag, wave, scheme=name)
        out[f"scheme_{name}_classic_rk4_3"] = np.stack([jvp(rollout(stepper, eq, dt, 3), u0[s], du[s], like) for s in range(2)])
    assert np.array_equal(out["scheme_van_leer_classic_rk4_3"], out["n16_b2_classic_rk4_3"])

    # degenerate starts: the limiter's ties
    n, dt = int(edges["n"]), float(edges["a1_dt"])
    like = like_of(n)
    eq, stepper = equation(n, "forward_euler", float(edges["a1_nu"]), float(edges["a1_drag"]), int(edges["wave"]))
    for si, start in enumerate(F.EDGE_STARTS):
        u0 = edges[f"a1_{start}_u0"]
        du = out[f"a1_{start}_du"] = perturbation((2, n, n), 330 + si)
        out[f"a1_{start}_explicit_jvp"] = jvp(lambda v: eq.explicit_terms(v, dt), u0, du, like)
        out[f"a1_{start}_forward_euler_jvp"] = jvp(rollout(stepper, eq, dt, 1), u0, du, like)

    # fp32 fields
    torch.set_default_dtype(torch.float32)
    eq, stepper = equation(32, "classic_rk4", nu, drag, wave)
    like = like_of(32)
    out["f32_du"] = perturbation((1, 2, 32, 32), 340, torch.float32)
    out["f32_classic_rk4_3"] = jvp(rollout(stepper, eq, float(grad["f32_dt"]), 3), grad["f32_u0"][0], out["f32_du"][0], like)[None]
    torch.set_default_dtype(torch.float64)
    assert out["f32_classic_rk4_3"].dtype == np.float32 and grad["f32_u0"].dtype == np.float32

    for k, v in out.items():
        assert v.dtype.kind == "f" and np.isfinite(v).all(), k
    path = os.path.join(HERE, "fvm_jvp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k, v in out.items():
        print(f"{k:36s} {v.dtype} {v.shape} max={np.abs(v).max():.3e}")
