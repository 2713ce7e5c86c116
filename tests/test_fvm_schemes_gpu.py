"""GPU tests of the finite-volume solver's selectable advection schemes (the SCHEME instantiations of k_fvm_stage and
k_fvm_stage_vjp in tcfd_fvm.hip) against the reference's goldens tests/golden/fvm_schemes_<scheme>.npz and the plain-torch
restatement tests/fvm_schemes_ops.py.  Bounds: those of tests/test_fvm_gpu.py and tests/test_fvm_grad_gpu.py for the same
quantities (explicit terms 1e-12, steps 1e-11, gradients 1e-10, fp32 2e-6 / 1e-5), on every cell."""
import math

import numpy as np
import pytest
import torch

import fvm_ops as F
import fvm_schemes_ops as S
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
L = 2 * math.pi
DEV = "cuda:0"
STARTS = F.EDGE_STARTS + ("smooth",)
NEW = ("upwind", "linear", "lax_wendroff")
FP64_BOUND = 1e-10   # tests/test_fvm_grad_gpu.py
METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")


@pytest.fixture
def fp64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _golden(scheme):
    return load_golden(f"fvm_schemes_{scheme}.npz")


def _golden_physics(g, scheme):
    return S.Physics(scheme, int(g["n"]), nu=float(g["nu"]), drag=float(g["drag"]), wave=int(g["wave"]))


def _stepper(method="classic_rk4"):
    import torch_cfd_amd as tc

    return tc.RKStepper.from_method(method=method)


def _dev(a, dtype=torch.float64):
    a = torch.as_tensor(np.asarray(a)).to(DEV, dtype)
    return a[..., 0, :, :].contiguous(), a[..., 1, :, :].contiguous()


def _leaves(a, dtype=torch.float64):
    return tuple(c.clone().requires_grad_() for c in _dev(a, dtype))


def _cpu(u):
    return torch.stack([c.detach().cpu() for c in u], dim=-3)


def _dot(out, cot):
    return (out[0] * cot[..., 0, :, :]).sum() + (out[1] * cot[..., 1, :, :]).sum()


def _vjp(fn, u, cot):
    cot = torch.as_tensor(np.asarray(cot)).to(DEV, u[0].dtype)
    return torch.stack(torch.autograd.grad(_dot(fn(u), cot), u), dim=-3)


def _finite(u):
    return all(torch.isfinite(c).all().item() for c in u)


def _err(got, want, n):
    """rel-L2 of the whole field and, where the last 64-wide x-block is partly masked, of its columns alone: every cell counts."""
    got = torch.stack(tuple(got), dim=-3).detach().cpu() if isinstance(got, tuple) else got.detach().cpu()
    want = torch.stack(tuple(want), dim=-3).detach().cpu() if isinstance(want, tuple) else want.detach().cpu()
    errs = [rel_l2(got, want)]
    if n > 64 and n % 64:
        errs.append(rel_l2(got[..., :, 64:], want[..., :, 64:]))
    return max(errs)


def _smooth(ph, seeds, dtype=torch.float64):
    from torch_cfd_amd import initial_conditions as ic

    ux, uy = ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=DEV, batch_seeds=list(seeds))
    return ux.detach().to(dtype), uy.detach().to(dtype)


def _edge_batch(n):
    """The four degenerate starts (faces with w == 0 and d == 0 exactly) as one batch of four."""
    u = torch.stack([F.degenerate_start(name, n, seed=n + k) for k, name in enumerate(F.EDGE_STARTS)])
    return u[:, 0].contiguous().to(DEV), u[:, 1].contiguous().to(DEV)


def _grad_leaves(u):
    return tuple(c.detach().clone().requires_grad_() for c in u)


def _equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------- against the reference's goldens (n = 16)
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_forward_against_the_reference(scheme, start, fp64_default):
    """The advection term alone, the explicit terms, 1 and 3 RK4 steps; the edge starts have faces with w == 0 (the c1
    branch) and d == 0."""
    g = _golden(scheme)
    ph, dt = _golden_physics(g, scheme), float(g["dt"])
    eq = ph.equation(_stepper())
    u0 = _dev(g[f"{start}_u0"])
    with torch.no_grad():
        c = eq.convect(u0, dt)
        k = eq.explicit_terms(u0, dt)
        u1 = eq(u0, dt)
        u3 = eq(u0, dt, steps=3)
    assert _finite(c) and _finite(k) and _finite(u1) and _finite(u3)
    errs = (rel_l2(_cpu(c), g[f"{start}_convect"]), rel_l2(_cpu(k), g[f"{start}_explicit"]),
            rel_l2(_cpu(u1), g[f"{start}_classic_rk4_1"]), rel_l2(_cpu(u3), g[f"{start}_classic_rk4_3"]))
    print(f"{scheme} {start}: convect {errs[0]:.2e}, explicit {errs[1]:.2e}, 1 step {errs[2]:.2e}, 3 steps {errs[3]:.2e}")
    assert errs[0] <= 1e-12 and errs[1] <= 1e-12, errs
    assert errs[2] <= 1e-11 and errs[3] <= 1e-11, errs


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_gradients_against_the_reference(scheme, start, fp64_default):
    """VJPs of the explicit terms and of one forward Euler step (whose explicit terms see the exact input: the ties), and of 3
    RK4 steps from the smooth start."""
    g = _golden(scheme)
    ph, dt = _golden_physics(g, scheme), float(g["dt"])
    cot = g[f"{start}_cot"]
    eq = ph.equation(_stepper("forward_euler"))
    cases = [("explicit_vjp", lambda u: eq.explicit_terms(u, dt)), ("forward_euler_vjp", lambda u: eq(u, dt))]
    if start == "smooth":
        rk4 = ph.equation(_stepper())
        cases.append(("classic_rk4_3_vjp", lambda u: rk4(u, dt, steps=3)))
    for key, fn in cases:
        got = _vjp(fn, _leaves(g[f"{start}_u0"]), cot)
        assert torch.isfinite(got).all()
        err = rel_l2(got.cpu(), g[f"{start}_{key}"])
        print(f"{scheme} {start} {key}: rel-L2 {err:.2e}")
        assert err <= FP64_BOUND, (key, err)


# ----------------------------------------------------------------------------- other sizes against the restatement
@pytest.mark.parametrize("n, batch", [(8, 2), (80, 3)])
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_other_sizes_against_the_restatement(scheme, n, batch, fp64_default):
    """n = 8: the stencil wraps onto itself; n = 80, batch 3: the last 64-wide x-block is partly masked and the transform is
    not a power of two.  A smooth batch and the batch of the four degenerate starts: forward and gradients.
    The flux's derivative with respect to the face velocity jumps at w == 0 (by c0 - c1 for upwind), and a stage state that
    is zero in exact arithmetic leaves the projection as transform roundoff of either sign.  So from the degenerate starts
    the gradients compared are those whose explicit terms see the exact input -- the terms themselves and one forward Euler
    step, as tests/test_fvm_grad_gpu.py does at the limiter's ties -- and the 3-step RK4 gradient is taken from the smooth
    start."""
    ph = S.Physics(scheme, n)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    a, b = eq.solver.weights(dt)
    euler = ph.equation(_stepper("forward_euler"))
    ea, eb = euler.solver.weights(dt)
    for tag, u0 in (("smooth", _smooth(ph, range(batch))), ("edges", _edge_batch(n))):
        nb = u0[0].shape[0]
        with torch.no_grad():
            checks = (("convect", eq.convect(u0, dt), ph.convect(dt)(u0), 1e-12),
                      ("explicit", eq.explicit_terms(u0, dt), ph.explicit(dt, DEV)(u0), 1e-12),
                      ("3 steps", eq(u0, dt, steps=3), ph.rollout(a, b, dt, 3, DEV)(u0), 1e-11))
        for what, got, want, bound in checks:
            err = _err(got, want, n)
            print(f"{scheme} n={n} {tag} {what}: rel-L2 {err:.2e}")
            assert _finite(got) and err <= bound, (tag, what, err)
        cot = F.cotangent((nb, 2, n, n), 7 * n)
        stepped = (("3 steps", lambda v: eq(v, dt, steps=3), ph.rollout(a, b, dt, 3, DEV)) if tag == "smooth" else
                   ("1 Euler step", lambda v: euler(v, dt), ph.rollout(ea, eb, dt, 1, DEV)))
        for what, fn, ops in (("convect", lambda v: eq.convect(v, dt), ph.convect(dt)),
                              ("explicit", lambda v: eq.explicit_terms(v, dt), ph.explicit(dt, DEV)), stepped):
            got, want = _vjp(fn, _grad_leaves(u0), cot), _vjp(ops, _grad_leaves(u0), cot)
            err = _err(got, want, n)
            print(f"{scheme} n={n} {tag} {what} VJP: rel-L2 {err:.2e}")
            assert torch.isfinite(got).all() and err <= FP64_BOUND, (tag, what, err)


@pytest.mark.parametrize("scheme", NEW)
def test_a_sample_in_a_ragged_batch_evolves_as_it_does_alone(scheme, fp64_default):
    n, batch = 32, 17
    ph = S.Physics(scheme, n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u0 = _smooth(ph, range(batch))
    cot = F.cotangent((batch, 2, n, n), batch)
    with torch.no_grad():
        out = eq(u0, dt, steps=3)
    grad = _vjp(lambda v: eq(v, dt, steps=3), _grad_leaves(u0), cot)
    assert out[0].shape == (batch, n, n)
    for s in (0, 8, batch - 1):
        one = (u0[0][s].contiguous(), u0[1][s].contiguous())
        with torch.no_grad():
            alone = eq(one, dt, steps=3)
        assert torch.equal(out[0][s], alone[0]) and torch.equal(out[1][s], alone[1]), s
        assert torch.equal(grad[s], _vjp(lambda v: eq(v, dt, steps=3), _grad_leaves(one), cot[s])), s


@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_named_methods_and_custom_tableaux_against_the_restatement(scheme, fp64_default):
    """Every named method and the general tableaux of fvm_ops.TABLEAUX, one step forward and its gradient, at n = 16."""
    import torch_cfd_amd as tc

    n = 16
    ph = S.Physics(scheme, n)
    dt = 0.25 * ph.h
    u0 = _smooth(ph, [0, 1])
    cot = F.cotangent((2, 2, n, n), 16)
    solvers = [(m, _stepper(m)) for m in METHODS] + [(t, tc.RKStepper(tableau=F.TABLEAUX[t], dtype=torch.float64)) for t in F.TABLEAUX]
    for name, solver in solvers:
        eq = ph.equation(solver)
        a, b = solver.weights(dt)
        with torch.no_grad():
            err = _err(eq(u0, dt), ph.rollout(a, b, dt, 1, DEV)(u0), n)
        assert err <= 1e-11, (name, err)
        err = _err(_vjp(lambda v: eq(v, dt), _grad_leaves(u0), cot), _vjp(ph.rollout(a, b, dt, 1, DEV), _grad_leaves(u0), cot), n)
        assert err <= FP64_BOUND, (name, err)


# ----------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_fp32_against_the_reference(scheme):
    g = _golden(scheme)
    ph = S.Physics(scheme, int(g["f32_n"]), nu=float(g["nu"]), drag=float(g["drag"]), wave=int(g["f32_wave"]))
    eq, dt = ph.equation(_stepper()), float(g["f32_dt"])
    u0 = _dev(g["f32_v0"], torch.float32)
    with torch.no_grad():
        k = eq.explicit_terms(u0, dt)
        u1 = eq(u0, dt)
        u10 = eq(u0, dt, steps=10)
    assert k[0].dtype == torch.float32 and u10[0].dtype == torch.float32
    errs = (rel_l2(_cpu(k), g["f32_explicit"]), rel_l2(_cpu(u1), g["f32_classic_rk4_1"]), rel_l2(_cpu(u10), g["f32_classic_rk4_10"]))
    print(f"{scheme} fp32: explicit {errs[0]:.2e}, 1 step {errs[1]:.2e}, 10 steps {errs[2]:.2e}")
    assert errs[0] <= 2e-6 and errs[1] <= 1e-5 and errs[2] <= 1e-5, errs
    # the fp32 adjoint runs and agrees with autograd through the fp32 restatement to fp32 rounding
    cot = F.cotangent((2, ph.n, ph.n), 64, torch.float32)
    got = _vjp(lambda v: eq.explicit_terms(v, dt), _grad_leaves(u0), cot)
    want = _vjp(ph.explicit(dt, DEV, torch.float32), _grad_leaves(u0), cot)
    assert got.dtype == torch.float32 and rel_l2(got.cpu(), want.cpu()) <= 1e-5


# ----------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("scheme", NEW)
def test_steps_k_under_grad_and_repeated_backward_are_bit_equal(scheme, fp64_default):
    import torch_cfd_amd as tc

    g = _golden(scheme)
    ph, dt = _golden_physics(g, scheme), float(g["dt"])
    eq = ph.equation(_stepper())
    u0 = _dev(g["smooth_u0"])
    with torch.no_grad():
        once = eq(u0, dt, steps=3)
        u = u0
        for _ in range(3):
            u = eq(u, dt)
        assert _equal(once, u)                                    # steps = 3 is three calls
        tx, ty = tc.get_trajectory_fvm(eq, u0, dt, num_steps=3, record_every_steps=1)
        assert torch.equal(tx[-1], once[0]) and torch.equal(ty[-1], once[1])
    leaves = _grad_leaves(u0)
    out = eq(leaves, dt, steps=3)
    assert out[0].requires_grad and _equal((out[0].detach(), out[1].detach()), once)   # forward under grad == no_grad
    cot = g["smooth_cot"]
    first = _vjp(lambda v: eq(v, dt, steps=3), _grad_leaves(u0), cot)
    again = _vjp(lambda v: eq(v, dt, steps=3), _grad_leaves(u0), cot)
    assert torch.equal(first, again)

    def chained(v):
        for _ in range(3):
            v = eq(v, dt)
        return v
    assert torch.equal(first, _vjp(chained, _grad_leaves(u0), cot))
    tx, ty = tc.get_trajectory_fvm(eq, _grad_leaves(u0), dt, num_steps=3, record_every_steps=3)
    assert tx.requires_grad and torch.equal(tx[0].detach(), once[0])


def test_the_default_path_is_unchanged(fp64_default):
    """convect omitted, None, fvm.convect and the explicitly limited Lax-Wendroff: one plan key, bit-identical results and
    gradients (and the goldens of the default, which tests/test_fvm_gpu.py holds them to)."""
    import torch_cfd_amd as tc
    from torch_cfd_amd import fvm, interpolation as I

    g = load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(g, "a1")
    dt = float(g["a1_dt"])
    grid = ph.grid()

    def build(**kw):
        forcing = tc.KolmogorovForcing(grid=grid, diam=ph.length, wave_number=ph.wave, offsets=grid.cell_faces)
        return tc.NavierStokes2DFVMProjection(ph.nu, grid, drag=ph.drag, forcing=forcing, solver=_stepper(), **kw)

    eqs = [build(), build(convect=None), build(convect=fvm.convect),
           build(convect=fvm.advection(I.apply_tvd_limiter(I.lax_wendroff, I.van_leer_limiter)))]
    keys = {eq._plan_key(torch.float64, torch.device(DEV))[:7] + eq._plan_key(torch.float64, torch.device(DEV))[9:] for eq in eqs}
    assert len(keys) == 1
    for name in ("integers", "blocks"):
        u0, cot = _dev(g[f"a1_{name}_u0"]), g[f"a1_{name}_cot"]
        outs, grads, terms = [], [], []
        for eq in eqs:
            with torch.no_grad():
                outs.append(eq(u0, dt, steps=3))
                terms.append(eq.explicit_terms(u0, dt))
            grads.append(_vjp(lambda v: eq(v, dt, steps=3), _grad_leaves(u0), cot))
        assert rel_l2(_cpu(outs[0]), g[f"a1_{name}_classic_rk4_3"]) <= 1e-11
        for k in range(1, len(eqs)):
            assert _equal(outs[0], outs[k]) and _equal(terms[0], terms[k]) and torch.equal(grads[0], grads[k]), k


def test_a_scheme_does_not_leak_into_another_equation_on_the_same_grid(fp64_default):
    g = _golden("upwind")
    dt = float(g["dt"])
    u0, cot = _dev(g["smooth_u0"]), g["smooth_cot"]
    up, vl = _golden_physics(g, "upwind").equation(_stepper()), _golden_physics(g, "van_leer").equation(_stepper())

    def alone(scheme):
        eq = _golden_physics(g, scheme).equation(_stepper())
        with torch.no_grad():
            out, terms = eq(u0, dt, steps=2), eq.explicit_terms(u0, dt)
        return out, terms, _vjp(lambda v: eq(v, dt, steps=2), _grad_leaves(u0), cot)
    want_up, want_vl = alone("upwind"), alone("van_leer")
    assert not _equal(want_up[0], want_vl[0])
    # interleaved calls, a pending backward of one across a forward of the other
    with torch.no_grad():
        a1 = up(u0, dt)
        b1 = vl(u0, dt)
        a2 = up(a1, dt)
        b2 = vl(b1, dt)
        ka, kb = up.explicit_terms(u0, dt), vl.explicit_terms(u0, dt)
    la, lb = _grad_leaves(u0), _grad_leaves(u0)
    oa = up(la, dt, steps=2)
    ob = vl(lb, dt, steps=2)
    cot_t = torch.as_tensor(cot).to(DEV)
    ga = torch.stack(torch.autograd.grad(_dot(oa, cot_t), la), dim=-3)
    gb = torch.stack(torch.autograd.grad(_dot(ob, cot_t), lb), dim=-3)
    assert _equal(a2, want_up[0]) and _equal(ka, want_up[1]) and torch.equal(ga, want_up[2])
    assert _equal(b2, want_vl[0]) and _equal(kb, want_vl[1]) and torch.equal(gb, want_vl[2])
    assert rel_l2(_cpu(ka), g["smooth_explicit"]) <= 1e-12
    assert rel_l2(_cpu(kb), _golden("van_leer")["smooth_explicit"]) <= 1e-12


def test_an_unknown_scheme_leaves_the_plan_as_it_was(fp64_default):
    import torch_cfd_amd as tc

    g = _golden("lax_wendroff")
    dt = float(g["dt"])
    eq = _golden_physics(g, "lax_wendroff").equation(_stepper())
    u0 = _dev(g["smooth_u0"])
    with torch.no_grad():
        before = eq.explicit_terms(u0, dt)
    plan = eq._plan(torch.float64, torch.device(DEV))
    lib = tc._lib.load()
    rc = lib.tcfd_fvm_plan_set_advection(plan.handle, 4)
    assert rc == -1 and b"scheme 4" in lib.tcfd_last_error()
    with torch.no_grad():
        assert _equal(before, eq.explicit_terms(u0, dt))
    assert rel_l2(_cpu(before), g["smooth_explicit"]) <= 1e-12
