#!/usr/bin/env python
"""Generate tests/golden/fvm_ensemble.npz -- an ensemble of finite-volume runs with per-member viscosity, drag and forcing
amplitude -- by IMPORTING THE REFERENCE (torch_cfd/fvm.py, pressure.py, forcings.py, initial_conditions.py).  Run inside the
build container only:

    python tests/golden/make_golden_fvm_ensemble.py

The reference has one physics per equation, so the ensemble is B = 4 SCALAR runs of it, stacked: n = 16, classic RK4, van
Leer advection, fp64, Kolmogorov forcing k = 2 of amplitude scale[b], dt = h / 4.

    nu, drag, scale         the members' values: distinct viscosities, one member WITHOUT drag, two equal forcing scales
    u0, du                  (B, 2, n, n): smooth starts (filtered_velocity_field, seeds 0..3) and seeded perturbations
    steps_1, steps_5        the state after 1 and 5 steps, member b from equation b
    tangent_1               the reference's forward-mode tangent of one step along du[b], member b from equation b
    margin_nu / margin_drag / margin_scale, tolerance
                            how far (rel-L2, the smallest over the members) the 5-step result moves when ONE member is given
                            its neighbour's viscosity, drag or forcing scale -- the neighbour being the next member, cyclically,
                            whose value differs -- and the tolerance of the GPU test.  The generator asserts that every margin
                            is at least 100 x the tolerance, and the same for a member run with member 0's whole physics: a
                            build that broadcasts one member's values cannot pass the test.

The file holds inputs and the reference's outputs, floating-point arrays only, no reference source; nothing at test time reads
the reference.  Deterministic (seeded CPU generators, fp64 CPU arithmetic).
"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from torch_cfd import boundaries, grids  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing  # noqa: E402
from torch_cfd.fvm import NavierStokes2DFVMProjection, RKStepper  # noqa: E402
from torch_cfd.initial_conditions import filtered_velocity_field  # noqa: E402

L = 2 * np.pi
N, WAVE = 16, 2
NU = [1e-2, 3e-3, 1e-3, 3e-4]
DRAG = [0.0, 0.1, 0.2, 0.05]
SCALE = [1.0, 1.0, 2.0, 0.5]
TOLERANCE = 1e-11   # rel-L2 of tests/test_fvm_gpu.py for its fp64 step goldens; tests/test_fvm_ensemble_gpu.py uses it


def grid_of(n):
    return grids.Grid((n, n), domain=((0, L), (0, L)))


def equation(nu, drag, scale):
    grid = grid_of(N)
    forcing = KolmogorovForcing(diam=L, wave_number=WAVE, grid=grid, scale=scale, offsets=((1.0, 0.5), (0.5, 1.0)))
    bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)
    stepper = RKStepper.from_method(method="classic_rk4", requires_grad=False, dtype=torch.float32)
    return NavierStokes2DFVMProjection(viscosity=nu, grid=grid, bcs=(bc, bc), density=1.0, drag=drag, forcing=forcing,
                                       solver=stepper), stepper


def arr(v):
    return np.stack([c.data.detach().cpu().numpy() for c in v])


def run(v, physics, dt, steps):
    eq, stepper = equation(*physics)
    with torch.no_grad():
        for _ in range(steps):
            v = stepper.forward(v, dt, equation=eq)
    return arr(v)


def tangent(like, u, du, physics, dt):
    eq, stepper = equation(*physics)
    with fwAD.dual_level():
        vs = [grids.GridVariable(grids.GridArray(fwAD.make_dual(torch.as_tensor(a).clone(), torch.as_tensor(d).clone()),
                                                 c.offset, c.grid), c.bc) for a, d, c in zip(u, du, like)]
        out = stepper.forward(grids.GridVariableVector(vs), dt, equation=eq)
        tangents = [fwAD.unpack_dual(c.data).tangent for c in out]
        assert all(t is not None for t in tangents)
        return np.stack([t.detach().numpy() for t in tangents])


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def differing_neighbour(values, b):
    for step in range(1, len(values)):
        if values[(b + step) % len(values)] != values[b]:
            return (b + step) % len(values)
    raise AssertionError("every member has the same value")


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B = len(NU)
    grid = grid_of(N)
    dt = 0.25 * min(grid.step)
    starts = [filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=s) for s in range(B)]
    du = torch.randn(B, 2, N, N, generator=torch.Generator().manual_seed(501), dtype=torch.float64).numpy()
    physics = [(NU[b], DRAG[b], SCALE[b]) for b in range(B)]
    out = {"n": N, "wave": WAVE, "dt": dt, "nu": np.array(NU), "drag": np.array(DRAG), "scale": np.array(SCALE),
           "u0": np.stack([arr(v) for v in starts]), "du": du, "tolerance": TOLERANCE}
    out["steps_1"] = np.stack([run(starts[b], physics[b], dt, 1) for b in range(B)])
    out["steps_5"] = np.stack([run(starts[b], physics[b], dt, 5) for b in range(B)])
    out["tangent_1"] = np.stack([tangent(starts[b], out["u0"][b], du[b], physics[b], dt) for b in range(B)])

    # one member with a neighbour's value of one parameter: the 5-step result must move by >= 100 x the tolerance
    for which, (name, values) in enumerate((("nu", NU), ("drag", DRAG), ("scale", SCALE))):
        moves = []
        for b in range(B):
            wrong = list(physics[b])
            wrong[which] = values[differing_neighbour(values, b)]
            moves.append(rel_l2(run(starts[b], tuple(wrong), dt, 5), out["steps_5"][b]))
        out[f"margin_{name}"] = min(moves)
        print(f"margin_{name}: {min(moves):.3e}  (per member {', '.join(f'{m:.2e}' for m in moves)})")
        assert min(moves) >= 100 * TOLERANCE, (name, moves)
    # a build that broadcasts member 0's physics to every member
    for b in range(1, B):
        move = rel_l2(run(starts[b], physics[0], dt, 5), out["steps_5"][b])
        assert move >= 100 * TOLERANCE, (b, move)

    for k, v in out.items():
        a = np.asarray(v)
        assert a.dtype.kind in "fi" and np.isfinite(a).all(), k
    path = os.path.join(HERE, "fvm_ensemble.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
