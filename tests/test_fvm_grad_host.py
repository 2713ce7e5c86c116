"""CPU tests of the finite-volume solver's reverse mode: torch autograd through the plain-torch restatement tests/fvm_ops.py
reproduces the reference's own autograd gradients (tests/golden/fvm_grad.npz), so it is a valid gradient oracle for the GPU
tests at sizes no golden covers; and the host logic of torch_cfd_amd/fvm_autograd.py."""
import math

import pytest
import torch

import fvm_ops as F
from conftest import load_golden, rel_l2

L = 2 * math.pi
METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")
CASES = ("n16_b2", "n32_b1")


def _golden():
    return load_golden("fvm_grad.npz")


def _leaves(a, dtype=torch.float64):
    t = torch.from_numpy(a).to(dtype)
    return t[..., 0, :, :].clone().requires_grad_(), t[..., 1, :, :].clone().requires_grad_()


def _vjp(fn, u, cot):
    out = fn(*u)
    cot = torch.as_tensor(cot).to(out[0].dtype)
    loss = (out[0] * cot[..., 0, :, :]).sum() + (out[1] * cot[..., 1, :, :]).sum()
    return torch.stack(torch.autograd.grad(loss, u), dim=-3)


def _rollout(n, method, k, dt, dtype=torch.float64):
    import torch_cfd_amd as tc

    a, b = tc.RKStepper.from_method(method=method).weights(dt)
    force = tuple(f.to(dtype) for f in F.kolmogorov_staggered(n, 4))
    inv = F.inverse_eigenvalues(n, L / n, dtype)

    def run(ux, uy):
        for _ in range(k):
            ux, uy = F.step(ux, uy, dt, a, b, L / n, 1e-3, 0.1, force, inv)
        return ux, uy
    return run


def test_restatement_explicit_terms_and_projection_vjps_against_the_reference():
    g = _golden()
    n = 32
    h = L / n
    dt = float(g["terms_dt"])
    force = F.kolmogorov_staggered(n, int(g["wave"]))
    got = _vjp(lambda x, y: F.explicit_terms(x, y, dt, h, float(g["nu"]), float(g["drag"]), force),
               _leaves(g["terms_u"]), g["terms_cot"])
    assert rel_l2(got, g["terms_explicit_vjp"]) <= 1e-13
    got = _vjp(lambda x, y: F.project(x, y, h, F.inverse_eigenvalues(n, h)), _leaves(g["proj_u"]), g["terms_cot"])
    assert rel_l2(got, g["proj_vjp"]) <= 1e-13


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("k", [1, 3])
def test_restatement_step_gradients_against_the_reference(case, method, k):
    g = _golden()
    n = int(case[1:3])
    got = _vjp(_rollout(n, method, k, float(g[f"{case}_dt"])), _leaves(g[f"{case}_u0"]), g[f"{case}_cot"])
    assert rel_l2(got, g[f"{case}_{method}_{k}"]) <= 1e-12


def test_restatement_fp32_gradient_against_the_reference():
    """fp32 on both sides: against the fp64 gradient at the same (fp32) inputs, the restatement's fp32 gradient is within
    twice the reference's own fp32 spread."""
    g = _golden()
    dt = float(g["f32_dt"])
    exact = _vjp(_rollout(32, "classic_rk4", 3, dt), _leaves(g["f32_u0"]), g["f32_cot"])
    got = _vjp(_rollout(32, "classic_rk4", 3, dt, torch.float32), _leaves(g["f32_u0"], torch.float32), g["f32_cot"])
    assert got.dtype == torch.float32
    spread = rel_l2(g["f32_classic_rk4_3"], exact)
    assert 1e-9 < spread < 1e-4
    assert rel_l2(got, exact) <= 2 * spread


def test_projection_is_symmetric_and_idempotent():
    """The property the adjoint rests on: the VJP of the projection is the projection (n = 8, dense Jacobian)."""
    n = 8
    h = L / n
    inv = F.inverse_eigenvalues(n, h)

    def P(v):
        x, y = F.project(v[: n * n].view(n, n), v[n * n:].view(n, n), h, inv)
        return torch.cat([x.reshape(-1), y.reshape(-1)])

    J = torch.autograd.functional.jacobian(P, torch.zeros(2 * n * n, dtype=torch.float64))
    assert (J - J.T).abs().max().item() <= 1e-14
    assert (J @ J - J).abs().max().item() <= 1e-13


def test_cotangent_of_one_component_may_be_none():
    from torch_cfd_amd import fvm_autograd as A

    like = torch.empty((), dtype=torch.float64).expand(2, 8, 8)
    g = torch.ones(8, dtype=torch.float64).expand(2, 8, 8)   # what the backward of .sum() hands over: stride 0
    gx, gy = A.cotangent_pair(None, g, like)
    assert torch.equal(gx, torch.zeros(2, 8, 8, dtype=torch.float64)) and gx.is_contiguous()
    assert torch.equal(gy, torch.ones(2, 8, 8, dtype=torch.float64)) and gy.is_contiguous()
    gx, gy = A.cotangent_pair(g.float(), None, like)
    assert gx.dtype == torch.float64 and torch.equal(gy, torch.zeros_like(gy))


def test_grad_path_engages_only_in_grad_mode_with_a_state_that_requires_grad():
    from torch_cfd_amd import fvm_autograd as A

    u = torch.zeros(4, 4)
    r = torch.zeros(4, 4, requires_grad=True)
    assert not A.wants_grad(u, u)
    assert A.wants_grad(u, r) and A.wants_grad(r, u)
    with torch.no_grad():
        assert not A.wants_grad(r, r)


def test_requires_grad_tableau_still_raises_with_a_differentiable_state():
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(32, 32), domain=((0, L), (0, L)))
    eq = tc.NavierStokes2DFVMProjection(1e-3, grid, drag=0.1)
    s = tc.RKStepper.from_method(method="classic_rk4", requires_grad=True)
    u = (torch.zeros(32, 32, requires_grad=True), torch.zeros(32, 32, requires_grad=True))
    with pytest.raises(NotImplementedError):
        eq.advance(u, 0.01, solver=s)


def test_default_tableau_does_not_block_the_velocity_gradient():
    """requires_grad=False leaves the tableau's parameters out of autograd, so a state that requires grad gets past the
    tableau check (and, on the CPU, to the device check)."""
    import torch_cfd_amd as tc

    s = tc.RKStepper.from_method(method="classic_rk4")
    assert not any(p.requires_grad for p in s.parameters())
    grid = tc.Grid(shape=(32, 32), domain=((0, L), (0, L)))
    eq = tc.NavierStokes2DFVMProjection(1e-3, grid, drag=0.1, solver=s)
    u = (torch.zeros(32, 32, requires_grad=True), torch.zeros(32, 32, requires_grad=True))
    with pytest.raises(tc._lib.TcfdError):
        eq(u, 0.01)


# ----------------------------------------------------------------------------- the edges (tests/golden/fvm_edges.npz)
def _edge_vjp(fn, a, cot):
    return _vjp(lambda x, y: fn((x, y)), _leaves(a), cot)


@pytest.mark.parametrize("name", F.EDGE_STARTS)
def test_restatement_vjps_at_the_limiter_ties_against_the_reference(name):
    """Explicit terms and one forward Euler step: both see the exact input, so the ties are exact on both sides."""
    import torch_cfd_amd as tc

    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, "a1")
    dt = float(g["a1_dt"])
    u0, cot = g[f"a1_{name}_u0"], g[f"a1_{name}_cot"]
    got = _edge_vjp(ph.explicit(dt), u0, cot)
    assert torch.isfinite(got).all()
    assert rel_l2(got, g[f"a1_{name}_explicit_vjp"]) <= 1e-13
    a, b = tc.RKStepper.from_method(method="forward_euler").weights(dt)
    got = _edge_vjp(ph.rollout(a, b, dt, 1), u0, cot)
    assert torch.isfinite(got).all()
    assert rel_l2(got, g[f"a1_{name}_forward_euler_vjp"]) <= 1e-12


@pytest.mark.parametrize("tag", F.OPTIONAL_TERMS)
def test_restatement_optional_terms_gradient_against_the_reference(tag):
    import torch_cfd_amd as tc

    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, f"a2_{tag}")
    dt = float(g[f"a2_{tag}_dt"])
    a, b = tc.RKStepper.from_method(method="classic_rk4").weights(dt)
    got = _edge_vjp(ph.rollout(a, b, dt, 3), g[f"a2_{tag}_u0"], g[f"a2_{tag}_cot"])
    assert rel_l2(got, g[f"a2_{tag}_classic_rk4_3_vjp"]) <= 1e-12


@pytest.mark.parametrize("name", list(F.TABLEAUX))
def test_restatement_general_tableaux_gradient_against_the_reference(name):
    import torch_cfd_amd as tc

    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, "a3")
    dt = float(g["a3_dt"])
    a, b = tc.RKStepper(tableau=F.TABLEAUX[name], dtype=torch.float64).weights(dt)
    got = _edge_vjp(ph.rollout(a, b, dt, 3), g["a3_u0"], g["a3_cot"])
    assert rel_l2(got, g[f"a3_{name}_3_vjp"]) <= 1e-12
