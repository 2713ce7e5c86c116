#!/usr/bin/env python
"""Generate tests/golden/fvm_*.npz -- the finite-volume solver's golden vectors -- by IMPORTING THE REFERENCE
(torch_cfd/fvm.py, pressure.py, forcings.py, initial_conditions.py).  Run inside the build container only:

    python tests/golden/make_golden_fvm.py

The outputs hold inputs + the reference's outputs, no reference source; nothing at test / bench time reads the
reference.  Deterministic (seeded CPU generators, fp64 CPU arithmetic): a rerun rewrites the files bit for bit.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))   # tests/: fvm_ops holds the degenerate starts and the tableaux the tests share

from torch_cfd import boundaries, grids  # noqa: E402
from torch_cfd.equations import stable_time_step  # noqa: E402
from torch_cfd.forcings import KolmogorovForcing  # noqa: E402
from torch_cfd.fvm import NavierStokes2DFVMProjection, RKStepper, convect, diffuse_velocity  # noqa: E402
from torch_cfd.initial_conditions import filtered_velocity_field  # noqa: E402
from torch_cfd.pressure import PressureProjection  # noqa: E402

import fvm_ops as F  # noqa: E402

L = 2 * np.pi
METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")


def grid_of(n):
    return grids.Grid((n, n), domain=((0, L), (0, L)))


def arr(v):
    return np.stack([c.data.detach().cpu().numpy() for c in v])


def equation(n, nu, drag, wave, method, dtype=torch.float32):
    grid = grid_of(n)
    forcing = KolmogorovForcing(diam=L, wave_number=wave, grid=grid, offsets=((1.0, 0.5), (0.5, 1.0)))
    bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)
    stepper = RKStepper.from_method(method=method, requires_grad=False, dtype=dtype)
    return NavierStokes2DFVMProjection(viscosity=nu, grid=grid, bcs=(bc, bc), density=1.0, drag=drag, forcing=forcing,
                                       solver=stepper), stepper


def run(v, stepper, eq, dt, steps):
    with torch.no_grad():
        for _ in range(steps):
            v = stepper.forward(v, dt, equation=eq)
    return v


def tables():
    out = {}
    for n in (32, 64):
        grid = grid_of(n)
        for wave in (3, 4):
            for swap in (False, True):
                f = KolmogorovForcing(diam=L, wave_number=wave, grid=grid, offsets=((1.0, 0.5), (0.5, 1.0)), swap_xy=swap)
                fx, fy = f(grid, None)
                out[f"force_n{n}_k{wave}_swap{int(swap)}"] = np.stack([fx.data.numpy(), fy.data.numpy()])
        bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)
        proj = PressureProjection(grid=grid, bc=bc)
        out[f"inverse_n{n}"] = proj.solver.inverse.numpy()
    eq, _ = equation(64, 1e-3, 0.1, 3, "classic_rk4")
    sd = eq.state_dict()
    out["state_dict_keys"] = np.array(list(sd.keys()))
    out["state_dict_shapes"] = np.array([",".join(map(str, t.shape)) for t in sd.values()])
    out["state_dict_dtypes"] = np.array([str(t.dtype) for t in sd.values()])
    np.savez_compressed(os.path.join(HERE, "fvm_tables.npz"), **out)


def small():
    """n = 64, fp64 fields, ν = 1e-3, drag 0.1, Kolmogorov k = 4; v0 from filtered_velocity_field seeds 42, 0, 1."""
    n, nu, drag, wave = 64, 1e-3, 0.1, 4
    grid = grid_of(n)
    out = {"n": n, "nu": nu, "drag": drag, "wave": wave}
    dt = stable_time_step(dx=min(grid.step), max_velocity=2.0, max_courant_number=0.5, viscosity=nu)
    out["dt"] = dt
    seeds = (42, 0, 1)
    out["seeds"] = np.array(seeds)
    v0s = [filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=s) for s in seeds]
    out["v0"] = np.stack([arr(v) for v in v0s])
    eq, stepper = equation(n, nu, drag, wave, "classic_rk4")
    v0 = v0s[0]
    with torch.no_grad():
        out["convect"] = arr(convect(v0, dt))
        out["diffuse"] = arr(diffuse_velocity(v0, nu))
        out["explicit"] = arr(eq.explicit_terms(v0, dt))
        gen = torch.Generator().manual_seed(7)
        raw = [grids.GridVariable(grids.GridArray(torch.randn(n, n, generator=gen), c.offset, grid), c.bc) for c in v0]
        raw = grids.GridVariableVector(raw)
        out["proj_in"] = arr(raw)
        out["proj_out"] = arr(eq.pressure_projection(raw))
    np.savez_compressed(os.path.join(HERE, "fvm_small.npz"), **out)
    # one file per seed (each file stays well under the 1 MiB limit of a committed file)
    for si, v in enumerate(v0s):
        per = {}
        for m in METHODS:
            eq, stepper = equation(n, nu, drag, wave, m)
            v1 = run(v, stepper, eq, dt, 1)
            per[f"{m}_1"] = arr(v1)
            per[f"{m}_10"] = arr(run(v1, stepper, eq, dt, 9))
        np.savez_compressed(os.path.join(HERE, f"fvm_small_s{si}.npz"), **per)

    # fp32 fields (default dtype float32 throughout, as a float32 run of the reference)
    torch.set_default_dtype(torch.float32)
    grid = grid_of(n)
    v32 = filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=42)
    eq, stepper = equation(n, nu, drag, wave, "classic_rk4")
    o32 = {"dt": dt, "v0": arr(v32), "explicit": arr(eq.explicit_terms(v32, dt))}
    o32["classic_rk4_1"] = arr(run(v32, stepper, eq, dt, 1))
    o32["classic_rk4_10"] = arr(run(v32, stepper, eq, dt, 10))
    torch.set_default_dtype(torch.float64)
    np.savez_compressed(os.path.join(HERE, "fvm_small_f32.npz"), **o32)


def notebook():
    """Kolmogrov2d_rk4_fvm_forced_turbulence.ipynb: n = 256, seed 42, max velocity 3, k = 3, ν = 1e-3, drag 0.1."""
    n, nu = 256, 1e-3
    grid = grid_of(n)
    v0 = filtered_velocity_field(grid, 3.0, 3.0, iterations=3, random_state=42)
    dt = stable_time_step(dx=min(grid.step), max_velocity=3.0, max_courant_number=0.5, viscosity=nu)
    eq, stepper = equation(n, nu, 0.1, 3, "classic_rk4")
    # one file per array: a 256^2 fp64 velocity pair is 1 MiB, the size limit of a committed file.  The 1000-step state
    # is stored as an fp32 snapshot (the test's bound there, 1e-5, is far above fp32 rounding).
    def save(name, **a):
        np.savez_compressed(os.path.join(HERE, f"fvm_notebook_{name}.npz"), **a)

    a0 = arr(v0)
    save("v0x", dt=dt, data=a0[0])
    save("v0y", data=a0[1])
    v = v0
    done = 0
    for target in (20, 200, 1000):
        v = run(v, stepper, eq, dt, target - done)
        done = target
        a = arr(v)
        if target < 1000:
            save(f"v{target}x", data=a[0])
            save(f"v{target}y", data=a[1])
        else:
            save(f"v{target}", data=a.astype(np.float32))


def state_of(arrays, like, leaves=False):
    """GridVariableVector of the given arrays with the offsets and bcs of `like` (fresh leaves that require grad on request)."""
    vs = [grids.GridVariable(grids.GridArray(a.clone().requires_grad_(leaves), c.offset, c.grid), c.bc)
          for a, c in zip(arrays, like)]
    return grids.GridVariableVector(vs), [v.data for v in vs]


def vjp(fn, arrays, like, cot):
    """Gradient of sum(cot * fn(state)) with respect to the two velocity arrays."""
    v, leaves = state_of(arrays, like, leaves=True)
    out = fn(v)
    loss = sum((c.data * g).sum() for c, g in zip(out, cot))
    return np.stack([g.numpy() for g in torch.autograd.grad(loss, leaves)])


def edges():
    """n = 16, fp64: the van Leer limiter's ties (A1), the optional terms (A2) and general tableaux (A3).  Every entry
    stores its inputs, cotangent and dt beside the reference's results."""
    n, wave = 16, 2
    bc = boundaries.HomogeneousBoundaryConditions(((boundaries.BCType.PERIODIC,) * 2,) * 2)

    def build(length, nu, drag, density, forced, stepper):
        grid = grids.Grid((n, n), domain=((0, length), (0, length)))
        forcing = KolmogorovForcing(diam=length, wave_number=wave, grid=grid, offsets=((1.0, 0.5), (0.5, 1.0))) if forced else None
        eq = NavierStokes2DFVMProjection(viscosity=nu, grid=grid, bcs=(bc, bc), density=density, drag=drag, forcing=forcing,
                                         solver=stepper)
        return grid, eq

    def named(method):
        return RKStepper.from_method(method=method, requires_grad=False, dtype=torch.float32)

    def rollout(stepper, eq, dt, k):
        def fn(v):
            for _ in range(k):
                v = stepper.forward(v, dt, equation=eq)
            return v
        return fn

    out = {"n": n, "wave": wave, "starts": np.array(F.EDGE_STARTS)}
    # ---- A1: degenerate starts, nu = 1e-3, drag 0.1, Kolmogorov k = 2, dt = h / 4
    rk4, euler = named("classic_rk4"), named("forward_euler")
    grid, eq = build(L, 1e-3, 0.1, 1.0, True, rk4)
    like = filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=0)
    dt = 0.25 * min(grid.step)
    out["a1_dt"], out["a1_nu"], out["a1_drag"] = dt, 1e-3, 0.1
    for si, name in enumerate(F.EDGE_STARTS):
        u = F.degenerate_start(name, n, seed=100 + si)
        cot = F.cotangent((2, n, n), 200 + si)
        v, _ = state_of(u, like)
        out[f"a1_{name}_u0"] = u.numpy()
        out[f"a1_{name}_cot"] = cot.numpy()
        with torch.no_grad():
            out[f"a1_{name}_explicit"] = arr(eq.explicit_terms(v, dt))
            out[f"a1_{name}_classic_rk4_1"] = arr(run(v, rk4, eq, dt, 1))
            out[f"a1_{name}_classic_rk4_3"] = arr(run(v, rk4, eq, dt, 3))
        out[f"a1_{name}_explicit_vjp"] = vjp(lambda w: eq.explicit_terms(w, dt), u, like, cot)
        out[f"a1_{name}_forward_euler_vjp"] = vjp(rollout(euler, eq, dt, 1), u, like, cot)
    # ---- A2: optional terms, smooth start (seed 0), nu = 1e-2, no drag
    # ("negdrag": a negative drag is no drag, `if self.drag > 0`; only there does a drag term applied regardless show)
    for ti, (tag, length, density, forced, drag) in enumerate((("plain", L, 1.0, False, 0.0), ("dense", 1.0, 2.0, True, 0.0),
                                                                ("negdrag", L, 1.0, False, -0.1))):
        grid, eq = build(length, 1e-2, drag, density, forced, rk4)
        like = filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=0)
        u = torch.stack([c.data.detach() for c in like])
        dt = 0.25 * min(grid.step)
        cot = F.cotangent((2, n, n), 300 + ti)
        out[f"a2_{tag}_length"], out[f"a2_{tag}_density"], out[f"a2_{tag}_forced"] = length, density, forced
        out[f"a2_{tag}_nu"], out[f"a2_{tag}_drag"] = 1e-2, drag
        out[f"a2_{tag}_dt"], out[f"a2_{tag}_u0"], out[f"a2_{tag}_cot"] = dt, u.numpy(), cot.numpy()
        with torch.no_grad():
            out[f"a2_{tag}_explicit"] = arr(eq.explicit_terms(like, dt))
            out[f"a2_{tag}_classic_rk4_3"] = arr(run(like, rk4, eq, dt, 3))
        out[f"a2_{tag}_classic_rk4_3_vjp"] = vjp(rollout(rk4, eq, dt, 3), u, like, cot)
    # ---- A3: general tableaux (fp64 parameters), smooth start, the physics of A1
    grid, eq = build(L, 1e-3, 0.1, 1.0, True, None)
    like = filtered_velocity_field(grid, 2.0, 3.0, iterations=3, random_state=0)
    u = torch.stack([c.data.detach() for c in like])
    dt = 0.25 * min(grid.step)
    cot = F.cotangent((2, n, n), 400)
    out["a3_dt"], out["a3_u0"], out["a3_cot"] = dt, u.numpy(), cot.numpy()
    for name, tableau in F.TABLEAUX.items():
        stepper = RKStepper(tableau=tableau, dtype=torch.float64)
        s = len(tableau["b"])
        a = np.zeros((s, s))
        for i, row in enumerate(tableau["a"]):
            a[i + 1, :len(row)] = row
        out[f"a3_{name}_a"], out[f"a3_{name}_b"] = a, np.array(tableau["b"])
        out[f"a3_{name}_1"] = arr(run(like, stepper, eq, dt, 1))
        out[f"a3_{name}_3"] = arr(run(like, stepper, eq, dt, 3))
        out[f"a3_{name}_3_vjp"] = vjp(rollout(stepper, eq, dt, 3), u, like, cot)
    for k, v in out.items():
        a = np.asarray(v)
        assert a.dtype.kind in "US" or np.isfinite(a).all(), k
    np.savez_compressed(os.path.join(HERE, "fvm_edges.npz"), **out)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    tables()
    small()
    notebook()
    edges()
    for f in sorted(os.listdir(HERE)):
        if f.startswith("fvm_") and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
