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
