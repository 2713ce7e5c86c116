"""GPU tests of the finite-volume solver's forward mode (k_fvm_stage_jvp of tcfd_fvm.hip on a tangent plan, the tangent-linear
entry points of torch_cfd_amd/fvm.py) against the reference's own tangents (tests/golden/fvm_jvp.npz), forward AD through the
restatement tests/fvm_ops.py / tests/fvm_schemes_ops.py at the sizes no golden covers (tests/test_fvm_jvp_host.py licenses it),
the existing adjoint kernels and central differences.  FP64_BOUND is the reverse-mode tests' bound."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import fvm_jvp_ops as J
import fvm_ops as F
import fvm_schemes_ops as S
from conftest import load_golden, rel_l2
from guard_ops import Arena, Out, nbytes, run_guarded

pytestmark = pytest.mark.gpu
L = 2 * math.pi
DEV = "cuda:0"
FP64_BOUND = 1e-10
SIZES = (8, 16, 32, 80, 96, 128, 160, 192)   # every size family; at n = 8 the +-2 stencil wraps at its limit
TCFD_EINVAL = -1


@pytest.fixture
def fp64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _stepper(method="classic_rk4"):
    import torch_cfd_amd as tc

    return tc.RKStepper.from_method(method=method)


def _pair(a, dtype=torch.float64):
    return J.pair(a, DEV, dtype)


def _smooth(ph, seeds):
    from torch_cfd_amd import initial_conditions as ic

    ux, uy = ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=DEV, batch_seeds=list(seeds))
    return ux.detach().clone(), uy.detach().clone()


def _ops_tangent(fn, u, du):
    """Tangent of the restatement `fn` by dual numbers, on the GPU."""
    return J.jvp(fn, u, du)[1]


def _band_err(got, want, n):
    """rel-L2 of the whole field and, where the last 64-wide x-block is partly masked, of its columns alone (a pair each)."""
    got, want = J.stacked(got), J.stacked(want)
    errs = [rel_l2(got, want)]
    if n > 64 and n % 64:
        errs.append(rel_l2(got[..., :, 64:], want[..., :, 64:]))
    return max(errs)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- 1. the reference's tangents, fp64
def test_explicit_terms_and_projection_tangents_against_the_reference(fp64_default):
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    eq = F.Physics(32, wave=int(gr["wave"])).equation(_stepper())
    dt = float(gr["terms_dt"])
    k, dk = eq.explicit_terms_jvp(_pair(gr["terms_u"]), _pair(g["terms_du"]), dt)
    err = rel_l2(J.stacked(dk), g["terms_explicit_jvp"])
    print(f"explicit-terms tangent rel-L2 {err:.2e}")
    assert err <= FP64_BOUND, err
    assert _equal(k, eq.explicit_terms(_pair(gr["terms_u"]), dt))
    _, dp = J.jvp(eq.pressure_projection, _pair(gr["proj_u"]), _pair(g["proj_du"]))
    err = rel_l2(J.stacked(dp), g["proj_jvp"])
    print(f"projection tangent rel-L2 {err:.2e}")
    assert err <= FP64_BOUND, err


@pytest.mark.parametrize("case", J.CASES)
@pytest.mark.parametrize("method", J.METHODS)
def test_step_tangents_against_the_reference(case, method, fp64_default):
    """1 and 3 steps of every named method, Kolmogorov forcing, drag 0.1; the batch of two pairs is one device call."""
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    eq = F.Physics(int(case[1:3]), wave=int(gr["wave"])).equation(_stepper(method))
    dt = float(gr[f"{case}_dt"])
    for k in (1, 3):
        _, du = eq.tangent_step(_pair(gr[f"{case}_u0"]), _pair(g[f"{case}_du"]), dt, steps=k)
        err = rel_l2(J.stacked(du), g[f"{case}_{method}_{k}"])
        print(f"{case} {method} {k} steps: rel-L2 {err:.2e}")
        assert err <= FP64_BOUND, (k, err)


@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_scheme_tangents_against_the_reference(scheme, fp64_default):
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    eq = S.Physics(scheme, 16, wave=int(gr["wave"])).equation(_stepper())
    _, du = eq.tangent_step(_pair(gr["n16_b2_u0"]), _pair(g["n16_b2_du"]), float(gr["n16_b2_dt"]), steps=3)
    err = rel_l2(J.stacked(du), g[f"scheme_{scheme}_classic_rk4_3"])
    print(f"{scheme}: 3 RK4 steps rel-L2 {err:.2e}")
    assert err <= FP64_BOUND, err


# ----------------------------------------------------------------------------- 2. fp32
def test_fp32_tangent_within_the_reference_fp32_spread(fp64_default):
    """fp32 fields: the spread is the reference's own fp32 tangent against the fp64 tangent at the same (fp32) inputs."""
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    dt = float(gr["f32_dt"])
    ph = F.Physics(32, wave=int(gr["wave"]))
    eq = ph.equation(_stepper())
    a, b = eq.solver.weights(dt)
    exact = J.stacked(_ops_tangent(ph.rollout(a, b, dt, 3, DEV), _pair(gr["f32_u0"]), _pair(g["f32_du"])))
    spread = rel_l2(g["f32_classic_rk4_3"], exact)
    u, du = eq.tangent_step(_pair(gr["f32_u0"], torch.float32), _pair(g["f32_du"], torch.float32), dt, steps=3)
    assert du[0].dtype == torch.float32 and u[0].dtype == torch.float32
    err = rel_l2(J.stacked(du), exact)
    print(f"fp32: rel-L2 {err:.2e} against fp64, the reference's fp32 {spread:.2e}")
    assert err <= 2 * spread, (err, spread)


# ----------------------------------------------------------------------------- 3. degenerate starts: the limiter's ties
@pytest.mark.parametrize("name", F.EDGE_STARTS)
def test_limiter_tie_tangents_against_the_reference(name, fp64_default):
    """The tangents of the explicit terms and of one forward Euler step, whose explicit terms see the exact input.  Only here
    does w > 0 differ from w >= 0 and the d == 0 arm of safe_div carry no tangent."""
    g, e = load_golden("fvm_jvp.npz"), load_golden("fvm_edges.npz")
    ph = F.Physics.of_golden(e, "a1")
    dt = float(e["a1_dt"])
    eq = ph.equation(_stepper("forward_euler"))
    u, du = _pair(e[f"a1_{name}_u0"]), _pair(g[f"a1_{name}_du"])
    _, dk = eq.explicit_terms_jvp(u, du, dt)
    assert all(torch.isfinite(c).all() for c in dk)
    err = rel_l2(J.stacked(dk), g[f"a1_{name}_explicit_jvp"])
    print(f"{name}: explicit-terms tangent rel-L2 {err:.2e}")
    assert err <= FP64_BOUND, err
    _, dn = eq.tangent_step(u, du, dt)
    assert all(torch.isfinite(c).all() for c in dn)
    err = rel_l2(J.stacked(dn), g[f"a1_{name}_forward_euler_jvp"])
    print(f"{name}: forward-Euler-step tangent rel-L2 {err:.2e}")
    assert err <= FP64_BOUND, err


@pytest.mark.parametrize("n", [8, 32, 80, 96])
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_limiter_tie_tangents_at_other_sizes_against_the_restatement(scheme, n, fp64_default):
    ph = S.Physics(scheme, n)
    dt = 0.25 * ph.h
    eq = ph.equation(_stepper("forward_euler"))
    a, b = eq.solver.weights(dt)
    for name in F.EDGE_STARTS:
        u = _pair(F.degenerate_start(name, n, seed=n))
        du = J.perturbation((2, n, n), 11 * n, DEV)
        _, got = eq.explicit_terms_jvp(u, du, dt)
        assert all(torch.isfinite(c).all() for c in got), name
        err = _band_err(got, _ops_tangent(ph.explicit(dt, DEV), u, du), n)
        assert err <= FP64_BOUND, (name, "explicit terms", err)
        _, got = eq.tangent_step(u, du, dt)
        assert all(torch.isfinite(c).all() for c in got), name
        err = _band_err(got, _ops_tangent(ph.rollout(a, b, dt, 1, DEV), u, du), n)
        assert err <= FP64_BOUND, (name, "forward Euler step", err)


# ----------------------------------------------------------------------------- 4. every size family
@pytest.mark.parametrize("n", SIZES)
def test_every_size_family_tangents_against_the_restatement(n, fp64_default):
    """Smooth start, batch 2: the tangents of the explicit terms, the projection and 3 RK4 steps."""
    import torch_cfd_amd as tc

    ph = F.Physics(n, wave=4)
    eq = ph.equation(_stepper())
    dt = tc.stable_time_step(dx=ph.h, max_velocity=2.0, max_courant_number=0.5, viscosity=ph.nu)
    a, b = eq.solver.weights(dt)
    u = _smooth(ph, [3, 5])
    du = J.perturbation((2, 2, n, n), n, DEV)
    for what, got, ops in (("explicit terms", eq.explicit_terms_jvp(u, du, dt)[1], ph.explicit(dt, DEV)),
                           ("projection", J.jvp(eq.pressure_projection, u, du)[1], ph.projection(DEV)),
                           ("3 steps", eq.tangent_step(u, du, dt, steps=3)[1], ph.rollout(a, b, dt, 3, DEV))):
        err = _band_err(got, _ops_tangent(ops, u, du), n)
        print(f"n={n} {what}: tangent rel-L2 {err:.2e}")
        assert err <= FP64_BOUND, (what, err)


# ----------------------------------------------------------------------------- 5. optional terms, general tableaux
@pytest.mark.parametrize("case", list(F.OPTIONAL_TERMS) + list(F.TABLEAUX))
def test_optional_terms_and_tableaux_tangent_at_n80_batch_three_against_the_restatement(case, fp64_default):
    import torch_cfd_amd as tc

    e = load_golden("fvm_edges.npz")
    if case in F.TABLEAUX:
        ph, solver = F.Physics.of_golden(e, "a3", n=80), tc.RKStepper(tableau=F.TABLEAUX[case], dtype=torch.float64)
    else:
        ph, solver = F.Physics.of_golden(e, f"a2_{case}", n=80), _stepper()
    eq, dt = ph.equation(solver), 0.25 * ph.h
    a, b = solver.weights(dt)
    u = _smooth(ph, [0, 1, 2])
    du = J.perturbation((3, 2, 80, 80), 80, DEV)
    state, got = eq.tangent_step(u, du, dt, steps=3)
    err = _band_err(got, _ops_tangent(ph.rollout(a, b, dt, 3, DEV), u, du), 80)
    print(f"{case} at 80^2 x 3: 3-step tangent rel-L2 {err:.2e}")
    assert err <= FP64_BOUND, err
    assert _equal(state, eq(u, dt, steps=3))


# ----------------------------------------------------------------------------- 6. adjoint identity with the existing VJP
@pytest.mark.parametrize("n", [32, 80])
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_adjoint_identity_against_the_vjp_kernels(scheme, n, fp64_default):
    """<J v, g> = <v, J^T g> ties k_fvm_stage_jvp to k_fvm_stage_vjp with no oracle in between.  Each side may be off by
    FP64_BOUND relative to its own factors, hence the form of the bound."""
    ph = S.Physics(scheme, n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _smooth(ph, [1, 2])
    v = J.perturbation((2, 2, n, n), 3 * n, DEV)
    g = J.perturbation((2, 2, n, n), 5 * n, DEV)
    dot = lambda p, q: sum((x * y).sum() for x, y in zip(p, q)).item()
    norm = lambda p: math.sqrt(dot(p, p))
    for what, jvp, fn in (("explicit terms", lambda: eq.explicit_terms_jvp(u, v, dt)[1], lambda w: eq.explicit_terms(w, dt)),
                          ("3 steps", lambda: eq.tangent_step(u, v, dt, steps=3)[1], lambda w: eq(w, dt, steps=3))):
        jv = jvp()
        leaves = tuple(c.clone().requires_grad_() for c in u)
        out = fn(leaves)
        jtg = torch.autograd.grad(sum((o * c).sum() for o, c in zip(out, g)), leaves)
        lhs, rhs = dot(jv, g), dot(v, jtg)
        bound = FP64_BOUND * (norm(jv) * norm(g) + norm(v) * norm(jtg))
        print(f"{scheme} n={n} {what}: <Jv, g> {lhs:.12e}, <v, J^T g> {rhs:.12e}, bound {bound:.2e}")
        assert abs(lhs - rhs) <= bound, (what, lhs, rhs)


# ----------------------------------------------------------------------------- 7. central differences
def test_explicit_terms_tangent_against_central_differences(fp64_default):
    """<lam, J v> against <lam, (F(u + e v) - F(u - e v)) / 2e> on a smooth field, n = 32."""
    import torch_cfd_amd as tc

    n = 32
    ph = F.Physics(n, wave=4)
    eq = ph.equation(_stepper())
    ux, uy = _smooth(ph, [3])
    ux, uy = ux[0], uy[0]
    dt = tc.stable_time_step(dx=L / n, max_velocity=2.0, max_courant_number=0.5, viscosity=1e-3)
    x = (torch.arange(n, dtype=torch.float64, device=DEV) + 0.5) * (L / n)
    v = (torch.sin(x)[:, None] * torch.cos(2 * x)[None, :], torch.cos(3 * x)[:, None] * torch.sin(x)[None, :])
    lam = (torch.cos(x)[:, None] * torch.cos(x)[None, :], torch.sin(2 * x)[:, None] * torch.cos(x)[None, :])
    dot = lambda p, q: sum((a * b).sum() for a, b in zip(p, q)).item()
    _, dk = eq.explicit_terms_jvp((ux, uy), v, dt)
    e = 1e-6
    fp = eq.explicit_terms((ux + e * v[0], uy + e * v[1]), dt)
    fm = eq.explicit_terms((ux - e * v[0], uy - e * v[1]), dt)
    fd = (dot(fp, lam) - dot(fm, lam)) / (2 * e)
    ad = dot(dk, lam)
    print(f"directional derivative: tangent {ad:.12e}, central difference {fd:.12e}")
    assert abs(ad - fd) <= 1e-6 * abs(fd), (ad, fd)


# ----------------------------------------------------------------------------- 8. bitwise properties
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_bitwise_properties_of_the_tangent(scheme, fp64_default):
    """The state half is the plain call; two runs agree; the tangent is linear in du under a scaling by two and zero for a
    zero du; steps=K is K chained calls.  n = 80 x 3: a partly masked block, a batch that is no power of two."""
    n = 80
    ph = S.Physics(scheme, n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _smooth(ph, [0, 1, 2])
    du = J.perturbation((3, 2, n, n), 17, DEV)
    k, dk = eq.explicit_terms_jvp(u, du, dt)
    assert _equal(k, eq.explicit_terms(u, dt))
    out, dout = eq.tangent_step(u, du, dt, steps=3)
    assert _equal(out, eq(u, dt, steps=3))
    again = eq.tangent_step(u, du, dt, steps=3)
    assert _equal(out, again[0]) and _equal(dout, again[1])
    assert _equal(dk, eq.explicit_terms_jvp(u, du, dt)[1])
    twice = tuple(2 * c for c in du)
    assert _equal(tuple(2 * c for c in dk), eq.explicit_terms_jvp(u, twice, dt)[1])
    assert _equal(tuple(2 * c for c in dout), eq.tangent_step(u, twice, dt, steps=3)[1])
    zero = tuple(torch.zeros_like(c) for c in du)
    for t in (eq.explicit_terms_jvp(u, zero, dt)[1], eq.tangent_step(u, zero, dt, steps=3)[1]):
        assert all(bool((c == 0).all()) for c in t)
    cu, cdu = u, du
    for _ in range(3):
        cu, cdu = eq.tangent_step(cu, cdu, dt)
    assert _equal(out, cu) and _equal(dout, cdu)
    same, dsame = eq.tangent_step(u, du, dt, steps=0)
    assert _equal(same, u) and _equal(dsame, du)


@pytest.mark.parametrize("n, batch", [(32, 17), (80, 9)])
def test_tangent_of_a_sample_in_a_ragged_batch_is_that_of_the_sample_alone(n, batch, fp64_default):
    ph = F.Physics(n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _smooth(ph, range(batch))
    du = J.perturbation((batch, 2, n, n), batch, DEV)
    out, dout = eq.tangent_step(u, du, dt, steps=3)
    k, dk = eq.explicit_terms_jvp(u, du, dt)
    for s in (0, 8, batch - 1):
        us, dus = tuple(c[s].clone() for c in u), tuple(c[s].clone() for c in du)
        alone, dalone = eq.tangent_step(us, dus, dt, steps=3)
        assert alone[0].shape == (n, n)
        assert _equal(tuple(c[s] for c in out), alone) and _equal(tuple(c[s] for c in dout), dalone), s
        ka, dka = eq.explicit_terms_jvp(us, dus, dt)
        assert _equal(tuple(c[s] for c in k), ka) and _equal(tuple(c[s] for c in dk), dka), s


# ----------------------------------------------------------------------------- 9. dual numbers
def _unpack(out):
    parts = [fwAD.unpack_dual(o) for o in out]
    assert all(p.tangent is not None for p in parts)
    return tuple(p.primal for p in parts), tuple(p.tangent for p in parts)


def test_dual_inputs_return_the_bits_of_the_explicit_calls(fp64_default):
    import torch_cfd_amd as tc

    n = 32
    ph = S.Physics("lax_wendroff", n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _smooth(ph, [0, 1, 2])
    du = J.perturbation((3, 2, n, n), 23, DEV)
    step = eq.tangent_step(u, du, dt, steps=2)
    one = eq.tangent_step(u, du, dt)
    terms = eq.explicit_terms_jvp(u, du, dt)
    with fwAD.dual_level():
        d = tuple(fwAD.make_dual(a, t) for a, t in zip(u, du))
        for what, got, want in (("forward", eq(d, dt, steps=2), step), ("advance", eq.advance(d, dt, steps=2), step),
                                ("RKStepper.forward", eq.solver(d, dt, eq), one),
                                ("explicit_terms", eq.explicit_terms(d, dt), terms)):
            p, t = _unpack(got)
            assert _equal(p, want[0]) and _equal(t, want[1]), what
        # the advection term alone: the explicit terms of an equation without viscosity, drag and forcing
        bare = tc.NavierStokes2DFVMProjection(0.0, ph.grid(), convect=ph.descriptor())
        p, t = _unpack(eq.convect(d, dt))
        want = bare.explicit_terms_jvp(u, du, dt)
        assert _equal(p, want[0]) and _equal(t, want[1])
        assert _equal(p, eq.convect(u, dt))
        # the projection is linear: its tangent is the projection of the perturbation
        for proj in (eq.pressure_projection, tc.PressureProjection(ph.grid())):
            p, t = _unpack(proj(d))
            assert _equal(p, eq.pressure_projection(u)) and _equal(t, eq.pressure_projection(du))
        tx, ty = tc.get_trajectory_fvm(eq, d, dt, num_steps=4, record_every_steps=2)
        (px, py), (dx, dy) = _unpack((tx, ty))
        assert px.shape == (3, 2, n, n)
        two = eq.tangent_step(*step, dt, steps=2)
        for r, want in enumerate((step, two)):
            assert _equal((px[:, r], py[:, r]), want[0]) and _equal((dx[:, r], dy[:, r]), want[1]), r
        # a dual on one component only: the other counts as a zero tangent
        zero = torch.zeros_like(du[0])
        for comp, dd in ((0, (d[0], u[1])), (1, (u[0], d[1]))):
            only = (du[0], zero) if comp == 0 else (zero, du[1])
            p, t = _unpack(eq(dd, dt, steps=2))
            want = eq.tangent_step(u, only, dt, steps=2)
            assert _equal(p, want[0]) and _equal(t, want[1]), comp
            p, t = _unpack(eq.explicit_terms(dd, dt))
            assert _equal(t, eq.explicit_terms_jvp(u, only, dt)[1]), comp
    # plain calls after the dual ones never see the tangent plans
    assert _equal(eq(u, dt, steps=2), step[0])
    assert not any(p.tangent for p in eq._plans.values()) and all(p.tangent for p in eq._tangent_plans.values())


# ----------------------------------------------------------------------------- 10. refusals
def test_refusals_of_the_python_entry_points(fp64_default):
    import torch_cfd_amd as tc

    n = 16
    ph = F.Physics(n)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _smooth(ph, [0, 1])
    du = J.perturbation((2, 2, n, n), 1, DEV)
    r = tuple(c.clone().requires_grad_() for c in u)
    for fn in (lambda a, b: eq.tangent_step(a, b, dt), lambda a, b: eq.explicit_terms_jvp(a, b, dt)):
        with pytest.raises(NotImplementedError, match="forward mode over reverse mode"):
            fn(r, du)
        with pytest.raises(NotImplementedError, match="forward mode over reverse mode"):
            fn(u, tuple(c.clone().requires_grad_() for c in du))
        with pytest.raises(ValueError):
            fn(u, tuple(c[0] for c in du))
        with pytest.raises(ValueError):
            fn(u, tuple(c.float() for c in du))
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="forward mode over reverse mode"):
            eq((fwAD.make_dual(r[0], du[0]), r[1]), dt)
    trainable = tc.RKStepper.from_method(method="classic_rk4", requires_grad=True)
    with pytest.raises(NotImplementedError, match="tableau"):
        ph.equation(trainable).tangent_step(u, du, dt)
    with fwAD.dual_level(), pytest.raises(NotImplementedError, match="tableau"):
        trainable(tuple(fwAD.make_dual(a, t) for a, t in zip(u, du)), dt, eq)
    with torch.no_grad():   # in no-grad mode nothing is asked of autograd
        got = ph.equation(trainable).tangent_step(r, du, dt)
    assert _equal(got[1], eq.tangent_step(u, du, dt)[1])


def test_refusals_of_the_c_abi_leave_the_outputs_untouched(fp64_default):
    from torch_cfd_amd import _lib

    lib = _lib.load()
    n = 16
    ph = F.Physics(n)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    tangent, plain = eq._plan(torch.float64, DEV, tangent=True), eq._plan(torch.float64, DEV)
    a, b = eq.solver.weights(dt)
    ca, cb = _lib.darray(a), _lib.darray(b)
    ux, uy = _smooth(ph, [0, 1, 2])
    gx, gy = J.perturbation((3, 2, n, n), 2, DEV)
    ox, oy = torch.full_like(ux, 7.0), torch.full_like(uy, 7.0)
    ws = tangent.workspace(4, lib.tcfd_fvm_step_vjp_workspace_bytes(tangent.handle, 4))
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    P = lambda t: t.data_ptr()
    h = tangent.handle

    def refused(rc, word):
        torch.cuda.synchronize()
        msg = lib.tcfd_last_error().decode()
        assert rc == TCFD_EINVAL and word in msg, (rc, msg)
        assert bool((ox == 7.0).all()) and bool((oy == 7.0).all())

    with torch.cuda.device(torch.device(DEV)):
        refused(lib.tcfd_fvm_explicit_terms(h, P(ux), P(uy), P(ox), P(oy), 3, dt, stream), "pairs")
        refused(lib.tcfd_fvm_step(h, P(ux), P(uy), P(ox), P(oy), 3, 1, len(b), ca, cb, dt, P(ws), ws.numel(), stream), "pairs")
        refused(lib.tcfd_fvm_explicit_terms_vjp(h, P(ux), P(uy), P(gx), P(gy), P(ox), P(oy), 2, dt, stream), "tangent plan")
        saved = torch.stack([ux[:2], uy[:2]])[None].contiguous()
        refused(lib.tcfd_fvm_step_vjp(h, P(saved), P(gx), P(gy), P(ox), P(oy), 2, 1, len(b), ca, cb, dt, P(ws), ws.numel(), stream),
                "tangent plan")
        # a value other than 0 or 1 leaves either plan as it was
        refused(lib.tcfd_fvm_plan_set_tangent(h, 2), "on = 2")
        refused(lib.tcfd_fvm_plan_set_tangent(plain.handle, -1), "on = -1")
        refused(lib.tcfd_fvm_explicit_terms(h, P(ux), P(uy), P(ox), P(oy), 3, dt, stream), "pairs")
        assert lib.tcfd_fvm_explicit_terms(plain.handle, P(ux), P(uy), P(ox), P(oy), 3, dt, stream) == 0
    torch.cuda.synchronize()
    kx, ky = plain.explicit_terms(ux, uy, dt)
    assert torch.equal(ox, kx) and torch.equal(oy, ky)


# ----------------------------------------------------------------------------- 11. memory contract of the tangent plan
def _guard(what, ins, outs, call, need, baseline):
    """One guarded case by the protocol of tests/guard_ops.py (as tests/test_memory_contract_gpu.py runs it)."""
    from torch_cfd_amd import _lib

    dev = torch.device(DEV)
    regions = [(k, nbytes(t.dtype, t.shape)) for k, t in ins.items()]
    if need:
        regions.append(("ws", int(need)))
    regions += [(k, nbytes(o.dtype, o.shape)) for k, o in outs.items()]
    arena = Arena(dev, regions)

    def run(ws_bytes):
        with torch.cuda.device(dev):
            return call(arena.ptr, arena.ptr("ws") if need else arena.buf.data_ptr(), ws_bytes)

    return run_guarded(run, arena, ins, outs, "ws" if need else None, need=int(need or 0), baseline=baseline,
                       last_error=_lib.load().tcfd_last_error, what=what)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_memory_contract_of_the_tangent_plan(dtype, fp64_default):
    """tcfd_fvm_explicit_terms and tcfd_fvm_step on a tangent plan, batch 2 B = 4, n = 16: inputs unchanged, nothing outside
    the outputs and the workspace written, results independent of what the scratch held, bit-equal to the wrapper path; a
    short workspace returns TCFD_EWORKSPACE without touching an output."""
    from torch_cfd_amd import _lib

    lib = _lib.load()
    n, B2 = 16, 4
    ph = F.Physics(n)
    solver = __import__("torch_cfd_amd").RKStepper(tableau=F.TABLEAUX["ssprk3"], dtype=torch.float64)
    eq, dt = ph.equation(solver), 0.25 * ph.h
    plan = eq._plan(dtype, DEV, tangent=True)
    a, b = solver.weights(dt)
    ca, cb = _lib.darray(a), _lib.darray(b)
    u = _smooth(ph, [0, 1])
    du = J.perturbation((2, 2, n, n), 4, DEV)
    ux, uy = (torch.cat([s, d]).to(dtype).contiguous() for s, d in zip(u, du))
    o = Out(dtype, (B2, n, n))
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    h = plan.handle
    kx, ky = plan.explicit_terms(ux, uy, dt)
    _guard("tcfd_fvm_explicit_terms on a tangent plan", {"ux": ux, "uy": uy}, {"kx": o, "ky": o},
           lambda P, ws, nb: lib.tcfd_fvm_explicit_terms(h, P("ux"), P("uy"), P("kx"), P("ky"), B2, dt, stream()),
           None, {"kx": kx, "ky": ky})
    need = lib.tcfd_fvm_workspace_bytes(h, B2)
    assert need == lib.tcfd_fvm_workspace_bytes(eq._plan(dtype, DEV).handle, B2)   # the carve for 2 B holds both halves
    sx, sy = plan.step(ux, uy, dt, a, b, 2)
    _guard("tcfd_fvm_step on a tangent plan", {"ux": ux, "uy": uy}, {"ox": o, "oy": o},
           lambda P, ws, nb: lib.tcfd_fvm_step(h, P("ux"), P("uy"), P("ox"), P("oy"), B2, 2, 3, ca, cb, dt, ws, nb, stream()),
           need, {"ox": sx, "oy": sy})
