"""CPU tests of the finite-volume solver's forward mode: torch.autograd.forward_ad through the plain-torch restatement
(tests/fvm_ops.py, tests/fvm_schemes_ops.py) reproduces the reference's own tangents (tests/golden/fvm_jvp.npz), so it is a
valid tangent oracle for the GPU tests at sizes no golden covers; and the host logic of the tangent-linear entry points of
torch_cfd_amd/fvm.py.  The bounds are those of tests/test_fvm_grad_host.py for the same restatement."""
import math
import os

import numpy as np
import pytest
import torch

import fvm_jvp_ops as J
import fvm_ops as F
import fvm_schemes_ops as S
from conftest import GOLDEN, ROOT, load_golden, rel_l2

L = 2 * math.pi


def _golden():
    return load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")


def _weights(method, dt):
    import torch_cfd_amd as tc

    return tc.RKStepper.from_method(method=method).weights(dt)


def _tangent(fn, u, du):
    return J.stacked(J.jvp(fn, J.pair(u), J.pair(du))[1])


def test_golden_is_small_and_holds_floating_point_arrays_only():
    path = os.path.join(GOLDEN, "fvm_jvp.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path, allow_pickle=False)
    for k in g.files:
        assert g[k].dtype in (np.float64, np.float32) and g[k].ndim >= 3 and np.isfinite(g[k]).all(), k


def test_restatement_explicit_terms_and_projection_tangents_against_the_reference():
    g, gr = _golden()
    ph = F.Physics(32, wave=int(gr["wave"]))
    dt = float(gr["terms_dt"])
    err = rel_l2(_tangent(ph.explicit(dt), gr["terms_u"], g["terms_du"]), g["terms_explicit_jvp"])
    print(f"explicit terms: rel-L2 {err:.2e}")
    assert err <= 1e-13
    err = rel_l2(_tangent(ph.projection(), gr["proj_u"], g["proj_du"]), g["proj_jvp"])
    print(f"projection: rel-L2 {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("case", J.CASES)
@pytest.mark.parametrize("method", J.METHODS)
@pytest.mark.parametrize("k", [1, 3])
def test_restatement_step_tangents_against_the_reference(case, method, k):
    g, gr = _golden()
    dt = float(gr[f"{case}_dt"])
    ph = F.Physics(int(case[1:3]), wave=int(gr["wave"]))
    got = _tangent(ph.rollout(*_weights(method, dt), dt, k), gr[f"{case}_u0"], g[f"{case}_du"])
    err = rel_l2(got, g[f"{case}_{method}_{k}"])
    print(f"{case} {method} {k} steps: rel-L2 {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_restatement_scheme_tangents_against_the_reference(scheme):
    g, gr = _golden()
    dt = float(gr["n16_b2_dt"])
    ph = S.Physics(scheme, 16, wave=int(gr["wave"]))
    got = _tangent(ph.rollout(*_weights("classic_rk4", dt), dt, 3), gr["n16_b2_u0"], g["n16_b2_du"])
    err = rel_l2(got, g[f"scheme_{scheme}_classic_rk4_3"])
    print(f"{scheme}: rel-L2 {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", F.EDGE_STARTS)
def test_restatement_tangents_at_the_limiter_ties_against_the_reference(name):
    """Explicit terms and one forward Euler step: both see the exact input, so the ties are exact on both sides."""
    g, _ = _golden()
    e = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(e, "a1")
    dt = float(e["a1_dt"])
    u0, du = e[f"a1_{name}_u0"], g[f"a1_{name}_du"]
    got = _tangent(ph.explicit(dt), u0, du)
    assert torch.isfinite(got).all()
    assert rel_l2(got, g[f"a1_{name}_explicit_jvp"]) <= 1e-13
    got = _tangent(ph.rollout(*_weights("forward_euler", dt), dt, 1), u0, du)
    assert torch.isfinite(got).all()
    assert rel_l2(got, g[f"a1_{name}_forward_euler_jvp"]) <= 1e-12


def test_restatement_fp32_tangent_against_the_reference():
    """fp32 on both sides: against the fp64 tangent at the same (fp32) inputs, the restatement's fp32 tangent is within
    twice the reference's own fp32 spread."""
    g, gr = _golden()
    dt = float(gr["f32_dt"])
    a, b = _weights("classic_rk4", dt)
    ph = F.Physics(32, wave=int(gr["wave"]))
    exact = _tangent(ph.rollout(a, b, dt, 3), gr["f32_u0"], g["f32_du"])
    u, du = J.pair(gr["f32_u0"], dtype=torch.float32), J.pair(g["f32_du"], dtype=torch.float32)
    got = J.stacked(J.jvp(ph.rollout(a, b, dt, 3, dtype=torch.float32), u, du)[1])
    assert got.dtype == torch.float32 and g["f32_classic_rk4_3"].dtype == np.float32
    spread = rel_l2(g["f32_classic_rk4_3"], exact)
    assert 1e-9 < spread < 1e-4
    assert rel_l2(got, exact) <= 2 * spread


# ----------------------------------------------------------------------------- the C ABI's new symbol
def test_set_tangent_is_declared_and_mirrored():
    from torch_cfd_amd import _lib

    header = open(os.path.join(ROOT, "include", "tcfd.h")).read()
    assert "int tcfd_fvm_plan_set_tangent(tcfd_fvm_plan* plan, int on);" in header
    assert "#define TCFD_ABI_VERSION 13" in header and _lib.ABI_VERSION == 13
    res, args = _lib.SIGNATURES["tcfd_fvm_plan_set_tangent"]
    assert res is _lib.SIGNATURES["tcfd_fvm_plan_set_advection"][0] and args == _lib.SIGNATURES["tcfd_fvm_plan_set_advection"][1]
    # no new workspace-taking entry point and no new size query: the tangent plan goes through the existing ones
    assert sum(name.endswith("_workspace_bytes") for name in _lib.SIGNATURES) == 11


# ----------------------------------------------------------------------------- host logic of the Python entry points
def _equation(solver="classic_rk4", requires_grad=False):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(32, 32), domain=((0, L), (0, L)))
    s = None if solver is None else tc.RKStepper.from_method(method=solver, requires_grad=requires_grad)
    return tc.NavierStokes2DFVMProjection(1e-3, grid, drag=0.1, solver=s)


def _zeros(*shape, dtype=torch.float64, **kw):
    return (torch.zeros(*shape, dtype=dtype, **kw), torch.zeros(*shape, dtype=dtype, **kw))


def test_tangent_step_without_a_solver_raises():
    with pytest.raises(ValueError, match="RKStepper"):
        _equation(None).tangent_step(_zeros(32, 32), _zeros(32, 32), 0.01)


@pytest.mark.parametrize("call", ["explicit_terms_jvp", "tangent_step"])
def test_argument_checks_precede_any_device_call(call):
    """On CPU tensors a device call would raise TcfdError (no CPU fallback): every refusal below comes first, and in the order
    shapes and dtypes -> gradients -> tableau."""
    import torch_cfd_amd as tc

    eq = _equation(requires_grad=True)   # a tableau that requires grad: refused last
    fn = getattr(eq, call)
    u = _zeros(32, 32)
    with pytest.raises(ValueError, match="tangent must have the shape and dtype"):
        fn(u, _zeros(2, 32, 32), 0.01)
    with pytest.raises(ValueError, match="tangent must have the shape and dtype"):
        fn(u, _zeros(32, 32, dtype=torch.float32), 0.01)
    with pytest.raises(ValueError, match="n = 32"):
        fn(_zeros(16, 16), _zeros(16, 16), 0.01)
    with pytest.raises(ValueError):
        fn(u, (torch.zeros(32, 32, dtype=torch.float64),), 0.01)
    for bad_u, bad_du in ((_zeros(32, 32, requires_grad=True), u), (u, _zeros(32, 32, requires_grad=True))):
        with pytest.raises(NotImplementedError, match="forward mode over reverse mode is not implemented"):
            fn(bad_u, bad_du, 0.01)
        with pytest.raises(ValueError):   # the shape check still comes first
            fn(bad_u, _zeros(2, 32, 32), 0.01)
    if call == "tangent_step":
        with pytest.raises(NotImplementedError, match="tableau"):
            fn(u, u, 0.01)
        with torch.no_grad(), pytest.raises(tc._lib.TcfdError):   # nothing left to refuse: the device check
            fn(u, u, 0.01)
    else:
        with pytest.raises(tc._lib.TcfdError):
            fn(u, u, 0.01)


def test_dual_inputs_reach_the_tangent_path():
    """A dual number takes the tangent-linear route in every entry point (on the CPU: as far as the device check), also with
    a tangent on one component only; a state that requires grad next to a tangent is refused."""
    import torch.autograd.forward_ad as fwAD

    import torch_cfd_amd as tc

    eq = _equation()
    z = torch.zeros(32, 32, dtype=torch.float64)
    with fwAD.dual_level():
        d = fwAD.make_dual(z.clone(), torch.ones_like(z))
        for u in ((d, d), (d, z), (z, d)):
            for fn in (lambda v: eq(v, 0.01), lambda v: eq.explicit_terms(v, 0.01), lambda v: eq.convect(v, 0.01),
                       eq.pressure_projection, lambda v: eq.solver(v, 0.01, eq),
                       lambda v: tc.fvm.get_trajectory_fvm(eq, v, 0.01, 2, 1)):
                with pytest.raises(tc._lib.TcfdError):
                    fn(u)
        r = z.clone().requires_grad_()
        for fn in (lambda v: eq(v, 0.01), lambda v: eq.explicit_terms(v, 0.01), lambda v: eq.convect(v, 0.01),
                   eq.pressure_projection):
            with pytest.raises(NotImplementedError, match="forward mode over reverse mode"):
                fn((d, r))
