"""GPU tests of the finite-volume solver (tcfd_fvm.hip) against the reference's goldens and the plain-torch restatement
tests/fvm_ops.py."""
import math

import numpy as np
import pytest
import torch

import fvm_ops as F
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
L = 2 * math.pi
DEV = "cuda:0"
METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")


def _equation(n, method="classic_rk4", wave=4, nu=1e-3, drag=0.1, dtype=torch.float32):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=wave, offsets=grid.cell_faces)
    return tc.NavierStokes2DFVMProjection(nu, grid, drag=drag, forcing=forcing,
                                          solver=tc.RKStepper.from_method(method=method, dtype=dtype))


@pytest.fixture
def fp64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _pair(a, dtype=torch.float64):
    t = torch.from_numpy(np.asarray(a)).to(DEV, dtype)
    return t[..., 0, :, :], t[..., 1, :, :]


def _cpu(u):
    return torch.stack([c.cpu() for c in u], dim=-3)


def test_explicit_terms_and_projection_against_the_reference(fp64_default):
    g = load_golden("fvm_small.npz")
    eq = _equation(64)
    k = eq.explicit_terms(_pair(g["v0"][0]), float(g["dt"]))
    assert rel_l2(_cpu(k), g["explicit"]) <= 1e-12
    p = eq.pressure_projection(_pair(g["proj_in"]))
    assert rel_l2(_cpu(p), g["proj_out"]) <= 1e-12


def test_fp32_explicit_terms_and_steps_against_the_reference():
    g = load_golden("fvm_small_f32.npz")
    eq = _equation(64)
    u0 = _pair(g["v0"], torch.float32)
    assert rel_l2(_cpu(eq.explicit_terms(u0, float(g["dt"]))), g["explicit"]) <= 2e-6
    with torch.no_grad():
        u1 = eq(u0, float(g["dt"]))
        u10 = eq(u0, float(g["dt"]), steps=10)
    assert u1[0].dtype == torch.float32
    assert rel_l2(_cpu(u1), g["classic_rk4_1"]) <= 1e-5
    assert rel_l2(_cpu(u10), g["classic_rk4_10"]) <= 1e-5


@pytest.mark.parametrize("method", METHODS)
def test_steps_of_every_method_against_the_reference(method, fp64_default):
    g = load_golden("fvm_small.npz")
    s0 = load_golden("fvm_small_s0.npz")
    eq = _equation(64, method)
    u0 = _pair(g["v0"][0])
    with torch.no_grad():
        u1 = eq(u0, float(g["dt"]))
        u10 = eq(u1, float(g["dt"]), steps=9)
    assert rel_l2(_cpu(u1), s0[f"{method}_1"]) <= 1e-11
    assert rel_l2(_cpu(u10), s0[f"{method}_10"]) <= 1e-11


@pytest.mark.parametrize("method", METHODS)
def test_batch_of_three_seeds_equals_the_single_sample_goldens(method, fp64_default):
    g = load_golden("fvm_small.npz")
    eq = _equation(64, method)
    u0 = _pair(g["v0"])   # (3, n, n) each
    with torch.no_grad():
        u10 = eq(u0, float(g["dt"]), steps=10)
    out = _cpu(u10)
    for s in range(3):
        assert rel_l2(out[s], load_golden(f"fvm_small_s{s}.npz")[f"{method}_10"]) <= 1e-11


def test_steps_k_is_bit_equal_to_k_calls(fp64_default):
    g = load_golden("fvm_small.npz")
    eq = _equation(64)
    u0 = _pair(g["v0"])
    with torch.no_grad():
        once = eq(u0, float(g["dt"]), steps=5)
        u = u0
        for _ in range(5):
            u = eq(u, float(g["dt"]))
    assert torch.equal(once[0], u[0]) and torch.equal(once[1], u[1])


def test_stepper_forward_is_the_notebook_calling_convention(fp64_default):
    g = load_golden("fvm_small.npz")
    eq = _equation(64)
    u0 = _pair(g["v0"][0])
    with torch.no_grad():
        a = eq.solver.forward(u0, float(g["dt"]), equation=eq)
        b = eq(u0, float(g["dt"]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_notebook_run_against_the_reference(fp64_default):
    """n = 256, seed 42, ν = 1e-3, drag 0.1, k = 3, the notebook's dt: 20, 200 and 1000 classic RK4 steps.  The
    1000-step golden is an fp32 snapshot (rounding 6e-8, far under the bound)."""
    g0x, g0y = load_golden("fvm_notebook_v0x.npz"), load_golden("fvm_notebook_v0y.npz")
    dt = float(g0x["dt"])
    assert abs(dt - 0.0040906154343617095) < 1e-15
    eq = _equation(256, wave=3)
    u = (torch.from_numpy(g0x["data"]).to(DEV), torch.from_numpy(g0y["data"]).to(DEV))
    done = 0
    with torch.no_grad():
        for target, bound in ((20, 1e-10), (200, 1e-8), (1000, 1e-5)):
            u = eq(u, dt, steps=target - done)
            done = target
            if target < 1000:
                ref = np.stack([load_golden(f"fvm_notebook_v{target}{c}.npz")["data"] for c in "xy"])
            else:
                ref = load_golden("fvm_notebook_v1000.npz")["data"].astype(np.float64)
            err = rel_l2(_cpu(u), ref)
            assert err <= bound, (target, err)


@pytest.mark.parametrize("n", [256, 1024, 2048])
def test_projection_leaves_a_divergence_free_field(n, fp64_default):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    gen = torch.Generator().manual_seed(n)
    u = torch.randn(2, 2, n, n, generator=gen).to(DEV)
    p = tc.PressureProjection(grid)((u[:, 0], u[:, 1]))
    h = L / n
    div = (p[0] - torch.roll(p[0], 1, -2)) / h + (p[1] - torch.roll(p[1], 1, -1)) / h
    umax = torch.maximum(p[0].abs().max(), p[1].abs().max())
    assert div.abs().max().item() <= 1e-10 * umax.item() / h


@pytest.mark.parametrize("n", [512, 1024, 2048])
def test_large_grids_batch_two_against_the_restatement(n, fp64_default):
    from torch_cfd_amd import initial_conditions as ic
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    ux, uy = ic.filtered_velocity_field(grid, 2.0, 3.0, random_state=0, device=DEV, batch_seeds=[3, 5])
    eq = _equation(n, wave=4)
    dt = tc.stable_time_step(dx=L / n, max_velocity=2.0, max_courant_number=0.5, viscosity=1e-3)
    with torch.no_grad():
        out = eq((ux, uy), dt)
    a, b = eq.solver.weights(dt)
    force = tuple(f.to(DEV) for f in F.kolmogorov_staggered(n, 4))
    ref = F.step(ux, uy, dt, a, b, L / n, 1e-3, 0.1, force, F.inverse_eigenvalues(n, L / n).to(DEV))
    assert rel_l2(_cpu(out), _cpu(ref)) <= 1e-11


def test_trajectory_helper_equals_the_explicit_loop(fp64_default):
    import torch_cfd_amd as tc

    g = load_golden("fvm_small.npz")
    eq = _equation(64)
    u0 = _pair(g["v0"])
    dt = float(g["dt"])
    with torch.no_grad():
        tx, ty = tc.get_trajectory_fvm(eq, u0, dt, num_steps=12, record_every_steps=4)
        u = u0
        for r in range(3):
            for _ in range(4):
                u = eq.solver.forward(u, dt, equation=eq)
            assert torch.equal(tx[:, r], u[0]) and torch.equal(ty[:, r], u[1])
    assert tx.shape == (3, 3, 64, 64)


def test_requires_grad_tableau_raises_on_device(fp64_default):
    import torch_cfd_amd as tc

    g = load_golden("fvm_small.npz")
    eq = _equation(64)
    s = tc.RKStepper.from_method(method="classic_rk4", requires_grad=True)
    with pytest.raises(NotImplementedError):
        s.forward(_pair(g["v0"][0]), float(g["dt"]), equation=eq)
    with torch.no_grad():
        s.forward(_pair(g["v0"][0]), float(g["dt"]), equation=eq)   # grad mode off: runs


def test_default_offset_forcing_tables_are_unchanged(fp64_default):
    """Corner offsets (the spectral path's default) sample both components on one mesh, bit for bit as before."""
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(64, 64), domain=((0, L), (0, L)))
    for swap in (False, True):
        f = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=4, swap_xy=swap)
        fx, fy = f(grid)
        x, y = grid.mesh((0, 0))
        wave = torch.sin(4.0 * y) if not swap else torch.sin(4.0 * x)
        want = (wave, torch.zeros_like(wave)) if not swap else (torch.zeros_like(wave), wave)
        assert torch.equal(fx.data, want[0]) and torch.equal(fy.data, want[1])


# ----------------------------------------------------------------------------- the edges: limiter ties, every size family,
# optional terms, general tableaux, fp32 at the large transforms, batch independence, unsupported sizes
SIZES = (8, 16, 32, 80, 96, 128, 160, 192)   # every size family; 80, 96, 160, 192 leave the last 64-wide x-block partly masked


def _rk4(dtype=torch.float32):
    import torch_cfd_amd as tc

    return tc.RKStepper.from_method(method="classic_rk4", dtype=dtype)


def _smooth(ph, seeds, dtype=torch.float64):
    from torch_cfd_amd import initial_conditions as ic

    ux, uy = ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=DEV, batch_seeds=list(seeds))
    return ux.to(dtype), uy.to(dtype)


def _dev(a, dtype=torch.float64):
    a = torch.as_tensor(a).to(DEV, dtype)
    return a[..., 0, :, :].contiguous(), a[..., 1, :, :].contiguous()


def _finite(u):
    return all(torch.isfinite(c).all().item() for c in u)


def _band_ok(got, want, n, bound):
    """The bar on the whole field and, where the last x-block is partly masked, on its columns alone."""
    got, want = torch.stack(got), torch.stack(want)
    got, want = got.cpu(), want.cpu()
    errs = [rel_l2(got, want)]
    if n > 64 and n % 64:
        errs.append(rel_l2(got[..., :, 64:], want[..., :, 64:]))
    return max(errs) <= bound, errs


@pytest.mark.parametrize("name", F.EDGE_STARTS)
def test_limiter_ties_against_the_reference(name, fp64_default):
    """Degenerate starts (w == 0, d == 0 exactly on 16-100 % of the faces): explicit terms, 1 and 3 RK4 steps."""
    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, "a1")
    eq, dt = ph.equation(_rk4()), float(g["a1_dt"])
    u0 = _dev(g[f"a1_{name}_u0"])
    with torch.no_grad():
        k = eq.explicit_terms(u0, dt)
        u1 = eq(u0, dt)
        u3 = eq(u0, dt, steps=3)
    assert _finite(k) and _finite(u1) and _finite(u3)
    assert rel_l2(_cpu(k), g[f"a1_{name}_explicit"]) <= 1e-12
    assert rel_l2(_cpu(u1), g[f"a1_{name}_classic_rk4_1"]) <= 1e-11
    assert rel_l2(_cpu(u3), g[f"a1_{name}_classic_rk4_3"]) <= 1e-11
    if name == "rest":   # the forcing is sin(k y) e_x: nothing ever drives uy, and ux stays a function of y alone
        assert torch.equal(u3[1], torch.zeros_like(u3[1]))
        assert torch.equal(u3[0], u3[0][:1].expand_as(u3[0]))


@pytest.mark.parametrize("n", [8, 32, 80, 96])
@pytest.mark.parametrize("name", F.EDGE_STARTS)
def test_limiter_ties_at_other_sizes_against_the_restatement(name, n, fp64_default):
    ph = F.Physics(n)
    eq, dt = ph.equation(_rk4()), 0.25 * ph.h
    u0 = _dev(F.degenerate_start(name, n, seed=n))
    a, b = eq.solver.weights(dt)
    with torch.no_grad():
        k = eq.explicit_terms(u0, dt)
        u3 = eq(u0, dt, steps=3)
        ok, errs = _band_ok(k, ph.explicit(dt, DEV)(u0), n, 1e-12)
        assert _finite(k) and ok, errs
        ok, errs = _band_ok(u3, ph.rollout(a, b, dt, 3, DEV)(u0), n, 1e-11)
        assert _finite(u3) and ok, errs


@pytest.mark.parametrize("n", SIZES)
def test_every_size_family_against_the_restatement(n, fp64_default):
    """Smooth start, batch 2: explicit terms, projection (of a field that is not divergence free) and 3 RK4 steps."""
    import torch_cfd_amd as tc

    ph = F.Physics(n, wave=4)
    eq = ph.equation(_rk4())
    dt = tc.stable_time_step(dx=ph.h, max_velocity=2.0, max_courant_number=0.5, viscosity=ph.nu)
    u0 = _smooth(ph, [3, 5])
    raw = _dev(F.cotangent((2, 2, n, n), n))
    a, b = eq.solver.weights(dt)
    with torch.no_grad():
        ok, errs = _band_ok(eq.explicit_terms(u0, dt), ph.explicit(dt, DEV)(u0), n, 1e-12)
        assert ok, ("explicit terms", errs)
        p = eq.pressure_projection(raw)
        ok, errs = _band_ok(p, ph.projection(DEV)(raw), n, 1e-12)
        assert ok, ("projection", errs)
        ok, errs = _band_ok(eq(u0, dt, steps=3), ph.rollout(a, b, dt, 3, DEV)(u0), n, 1e-11)
        assert ok, ("3 steps", errs)
    if n in (80, 96):
        div = (p[0] - torch.roll(p[0], 1, -2)) / ph.h + (p[1] - torch.roll(p[1], 1, -1)) / ph.h
        umax = torch.maximum(p[0].abs().max(), p[1].abs().max())
        assert div.abs().max().item() <= 1e-10 * umax.item() / ph.h


@pytest.mark.parametrize("tag", F.OPTIONAL_TERMS)
def test_optional_terms_against_the_reference(tag, fp64_default):
    """No forcing (a null table) and no drag; density 2 on [0, 1]^2; a negative drag, which is no drag as in the reference."""
    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, f"a2_{tag}")
    eq, dt = ph.equation(_rk4()), float(g[f"a2_{tag}_dt"])
    u0 = _dev(g[f"a2_{tag}_u0"])
    with torch.no_grad():
        assert rel_l2(_cpu(eq.explicit_terms(u0, dt)), g[f"a2_{tag}_explicit"]) <= 1e-12
        assert rel_l2(_cpu(eq(u0, dt, steps=3)), g[f"a2_{tag}_classic_rk4_3"]) <= 1e-11


@pytest.mark.parametrize("name", list(F.TABLEAUX))
def test_general_tableaux_against_the_reference(name, fp64_default):
    """Stage states summed from two earlier stages, negative weights, a stage whose row is all zeros."""
    import torch_cfd_amd as tc

    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, "a3")
    eq, dt = ph.equation(tc.RKStepper(tableau=F.TABLEAUX[name], dtype=torch.float64)), float(g["a3_dt"])
    u0 = _dev(g["a3_u0"])
    with torch.no_grad():
        u1 = eq(u0, dt)
        u3 = eq(u0, dt, steps=3)
        assert rel_l2(_cpu(u1), g[f"a3_{name}_1"]) <= 1e-11
        assert rel_l2(_cpu(u3), g[f"a3_{name}_3"]) <= 1e-11
        if name == "zero_row":
            u = u1
            for _ in range(2):
                u = eq(u, dt)
            assert torch.equal(u3[0], u[0]) and torch.equal(u3[1], u[1])


@pytest.mark.parametrize("case", list(F.OPTIONAL_TERMS) + list(F.TABLEAUX))
def test_optional_terms_and_tableaux_at_n80_batch_three_against_the_restatement(case, fp64_default):
    import torch_cfd_amd as tc

    g = load_golden("fvm_edges.npz")
    if case in F.TABLEAUX:
        ph, solver = F.Physics.of_golden(g, "a3", n=80), tc.RKStepper(tableau=F.TABLEAUX[case], dtype=torch.float64)
    else:
        ph, solver = F.Physics.of_golden(g, f"a2_{case}", n=80), _rk4()
    eq, dt = ph.equation(solver), 0.25 * ph.h
    u0 = _smooth(ph, [0, 1, 2])
    a, b = solver.weights(dt)
    with torch.no_grad():
        ok, errs = _band_ok(eq.explicit_terms(u0, dt), ph.explicit(dt, DEV)(u0), 80, 1e-12)
        assert ok, ("explicit terms", errs)
        ok, errs = _band_ok(eq(u0, dt, steps=3), ph.rollout(a, b, dt, 3, DEV)(u0), 80, 1e-11)
        assert ok, ("3 steps", errs)


@pytest.mark.parametrize("n", [512, 1024])
def test_fp32_at_the_large_transforms_within_twice_the_torch_ops_fp32_error(n, fp64_default):
    """fp32 fields at the sizes whose transforms are the 8-column cross-lane tiles (1024: the cross-lane row kernel too).
    Truth: the restatement in fp64 on the same fp32 inputs cast up.  Yardstick: the restatement in float32 torch ops on the
    same device; the kernels may err at most twice as much (two fp32 pipelines order their sums differently).
    Measured on an MI355X, kernels / torch ops fp32 (rel-L2 for the step and the projection, max|div| h / max|u|):
        n = 512:   one RK4 step 5.54e-8 / 5.56e-8,  projection 4.46e-7 / 4.51e-7,  divergence 1.14e-6 / 1.10e-6
        n = 1024:  one RK4 step 5.79e-8 / 5.79e-8,  projection 4.91e-7 / 4.92e-7,  divergence 1.32e-6 / 1.27e-6"""
    import torch_cfd_amd as tc

    ph = F.Physics(n, wave=4)
    eq = ph.equation(_rk4())
    dt = tc.stable_time_step(dx=ph.h, max_velocity=2.0, max_courant_number=0.5, viscosity=ph.nu)
    a, b = eq.solver.weights(dt)
    u32 = _smooth(ph, [3, 5], torch.float32)
    raw32 = _dev(F.cotangent((2, 2, n, n), n), torch.float32)
    up = lambda u: tuple(c.double() for c in u)   # noqa: E731
    with torch.no_grad():
        got = eq(u32, dt)
        assert got[0].dtype == torch.float32
        exact = torch.stack(ph.rollout(a, b, dt, 1, DEV)(up(u32))).cpu()
        ops = torch.stack(ph.rollout(a, b, dt, 1, DEV, torch.float32)(u32)).cpu()
        assert ops.dtype == torch.float32
        err, spread = rel_l2(torch.stack(got).cpu(), exact), rel_l2(ops, exact)
        print(f"fp32 n={n} one RK4 step: kernels {err:.3e}, torch ops fp32 {spread:.3e}")
        assert err <= 2 * spread, ("step", err, spread)

        p = eq.pressure_projection(raw32)
        assert p[0].dtype == torch.float32
        exact = torch.stack(ph.projection(DEV)(up(raw32))).cpu()
        pops = ph.projection(DEV, torch.float32)(raw32)
        err, spread = rel_l2(torch.stack(p).cpu(), exact), rel_l2(torch.stack(pops).cpu(), exact)
        print(f"fp32 n={n} projection: kernels {err:.3e}, torch ops fp32 {spread:.3e}")
        assert err <= 2 * spread, ("projection", err, spread)

        def divergence(v):   # max|div| h / max|u| of an fp32 field, measured in fp64
            x, y = up(v)
            div = (x - torch.roll(x, 1, -2)) / ph.h + (y - torch.roll(y, 1, -1)) / ph.h
            return div.abs().max().item() * ph.h / max(x.abs().max().item(), y.abs().max().item())
        err, spread = divergence(p), divergence(pops)
        print(f"fp32 n={n} divergence after projection: kernels {err:.3e}, torch ops fp32 {spread:.3e}")
        assert err <= 2 * spread, ("divergence", err, spread)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n, batch", [(32, 17), (80, 9)])
def test_a_sample_in_a_ragged_batch_evolves_as_it_does_alone(n, batch, dtype, fp64_default):
    ph = F.Physics(n, wave=4)
    eq, dt = ph.equation(_rk4()), 0.25 * ph.h
    u0 = _smooth(ph, range(batch), dtype)
    with torch.no_grad():
        out = eq(u0, dt, steps=3)
        assert out[0].dtype == dtype and out[0].shape == (batch, n, n)
        for s in (0, 8, batch - 1):
            alone = eq((u0[0][s].contiguous(), u0[1][s].contiguous()), dt, steps=3)
            assert torch.equal(out[0][s], alone[0]) and torch.equal(out[1][s], alone[1]), s


@pytest.mark.parametrize("n", [100, 48])
def test_sizes_the_transforms_do_not_hold_raise_naming_the_size(n, fp64_default):
    """Even sizes the reference accepts and the transforms do not hold: an error that names n, not a crash or values."""
    import torch_cfd_amd as tc

    ph = F.Physics(n)
    u = tuple(torch.zeros(n, n, device=DEV) for _ in range(2))
    eq = ph.equation(_rk4())
    for call in (lambda: eq(u, 0.01), lambda: eq.explicit_terms(u, 0.01), lambda: eq.pressure_projection(u),
                 lambda: tc.PressureProjection(ph.grid())(u)):
        with pytest.raises(tc._lib.TcfdError, match=f"n={n}"):
            call()
