"""GPU tests of the finite-volume tangent bundle: K perturbations of one state through k_fvm_stage_jvp_bundle of tcfd_fvm.hip on
a bundle plan (tcfd_fvm_plan_set_tangent_bundle, include/tcfd_fvm_bundle.h) and the entry points ``tangent_bundle_step`` /
``explicit_terms_jvp_bundle`` of torch_cfd_amd/fvm.py.

The strongest check is bitwise: member k of a bundle call is ``torch.equal`` to ``tangent_step(u, dU[k])`` /
``explicit_terms_jvp(u, dU[k])``, the state half to the plain step.  Next to it the reference's own tangents
(tests/golden/fvm_jvp.npz) within FP64_BOUND, the bound of tests/test_fvm_jvp_gpu.py, and the dot-product identity against the
VJP kernels with that file's bound.

Sizes: n = 8 (the +-2 stencil wraps at its limit), 16, 80 (a full 64-wide block and a partly masked one), 96; B = 3, an odd batch;
K = 1 (the pair layout), 3 and 5."""
import ctypes
import math

import pytest
import torch

import fvm_jvp_ops as J
import fvm_ops as F
import fvm_schemes_ops as S
from conftest import load_golden, rel_l2
from guard_ops import TCFD_EWORKSPACE, Arena, Out, nbytes, run_guarded

pytestmark = pytest.mark.gpu
L = 2 * math.pi
DEV = "cuda:0"
FP64_BOUND = 1e-10          # tests/test_fvm_jvp_gpu.py
TCFD_EINVAL = -1
SIZES = (8, 16, 80, 96)
KS = (1, 3, 5)
DTYPES = (torch.float64, torch.float32)
B = 3


@pytest.fixture(autouse=True)
def fp64_default():
    """The grid and the forcing table are formed in the default dtype: fp64 (the fields of a test carry their own dtype)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _stepper(method="classic_rk4"):
    import torch_cfd_amd as tc

    return tc.RKStepper.from_method(method=method)


def _pair(a, dtype=torch.float64):
    return J.pair(a, DEV, dtype)


def _to(p, dtype):
    return tuple(c.to(dtype) for c in p)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _finite(p):
    return all(bool(torch.isfinite(c).all()) for c in p)


def _bundle(members):
    """K pairs -> the bundle (dVx, dVy), components (K,) + shape."""
    return tuple(torch.stack([m[c] for m in members]) for c in (0, 1))


def _member(dV, k):
    return tuple(c[k] for c in dV)


_SMOOTH = {}


def _smooth(n, batch=B):
    """A smooth (batch, n, n) fp64 velocity pair, made once per size."""
    if (n, batch) not in _SMOOTH:
        from torch_cfd_amd import initial_conditions as ic

        ux, uy = ic.filtered_velocity_field(F.Physics(n).grid(), 2.0, 3.0, random_state=0, device=DEV, batch_seeds=list(range(batch)))
        _SMOOTH[(n, batch)] = (ux.detach().double().clone(), uy.detach().double().clone())
    return _SMOOTH[(n, batch)]


def _members(n, count, batch=B, seed=0):
    """`count` seeded (batch, n, n) perturbation pairs."""
    return [J.perturbation((batch, 2, n, n), 1000 * seed + 31 * n + k, DEV) for k in range(count)]


def _check_bits_of_tangent_step(eq, u, members, dt, what):
    """Every member of the bundles of K in KS, on the explicit terms and on 3 steps, against the pair calls; the state half
    against the plain calls."""
    pairs = [(eq.explicit_terms_jvp(u, m, dt), eq.tangent_step(u, m, dt, steps=3)) for m in members]
    plain_k, plain_u = eq.explicit_terms(u, dt), eq(u, dt, steps=3)
    assert _finite(plain_u) and all(_finite(s[1]) for _, s in pairs), what
    for K in KS:
        dV = _bundle(members[:K])
        k, dK = eq.explicit_terms_jvp_bundle(u, dV, dt)
        out, dU = eq.tangent_bundle_step(u, dV, dt, steps=3)
        assert dK[0].shape == (K,) + tuple(u[0].shape) and dU[0].dtype == u[0].dtype
        assert _equal(k, plain_k) and _equal(out, plain_u), (what, K, "state")
        for m in range(K):
            (k1, dk1), (u1, du1) = pairs[m]
            assert _equal(_member(dK, m), dk1), (what, K, m, "explicit terms")
            assert _equal(_member(dU, m), du1), (what, K, m, "3 steps")
            assert _equal(k, k1) and _equal(out, u1)


# ----------------------------------------------------------------------------- 1. the reference's tangents, fp64
def _against_golden(dU, want, what):
    """Members 0 and 1 of a bundle (du, 2 du, third) against the golden tangent and twice it; member 1 is twice member 0."""
    want = torch.as_tensor(want)
    e0, e1 = rel_l2(J.stacked(_member(dU, 0)), want), rel_l2(J.stacked(_member(dU, 1)), 2 * want)
    print(f"{what}: rel-L2 {e0:.2e} (du), {e1:.2e} (2 du)")
    assert e0 <= FP64_BOUND and e1 <= FP64_BOUND, (what, e0, e1)
    assert _equal(_member(dU, 1), tuple(2 * c for c in _member(dU, 0))), what


def test_explicit_terms_bundle_against_the_reference():
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    eq = F.Physics(32, wave=int(gr["wave"])).equation(_stepper())
    u, du = _pair(gr["terms_u"]), _pair(g["terms_du"])
    third = _pair(torch.randn(2, 32, 32, generator=torch.Generator().manual_seed(5), dtype=torch.float64))
    dV = _bundle([du, tuple(2 * c for c in du), third])
    k, dK = eq.explicit_terms_jvp_bundle(u, dV, float(gr["terms_dt"]))
    assert dK[0].shape == (3, 32, 32)
    _against_golden(dK, g["terms_explicit_jvp"], "explicit terms")
    assert _equal(k, eq.explicit_terms(u, float(gr["terms_dt"])))


def _golden_bundle(g, gr):
    du = _pair(g["n16_b2_du"])
    third = J.perturbation((2, 2, 16, 16), 77, DEV)   # one golden tangent per state: the third member is random (checked in 2.)
    return _pair(gr["n16_b2_u0"]), _bundle([du, tuple(2 * c for c in du), third]), float(gr["n16_b2_dt"])


@pytest.mark.parametrize("method", J.METHODS)
def test_step_bundle_against_the_reference(method):
    """1 and 3 steps of every named method, Kolmogorov forcing, drag 0.1, the two states of n16_b2 in one call."""
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    eq = F.Physics(16, wave=int(gr["wave"])).equation(_stepper(method))
    u, dV, dt = _golden_bundle(g, gr)
    for k in (1, 3):
        _, dU = eq.tangent_bundle_step(u, dV, dt, steps=k)
        _against_golden(dU, g[f"n16_b2_{method}_{k}"], f"{method} {k} steps")


@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_scheme_bundle_against_the_reference(scheme):
    g, gr = load_golden("fvm_jvp.npz"), load_golden("fvm_grad.npz")
    eq = S.Physics(scheme, 16, wave=int(gr["wave"])).equation(_stepper())
    u, dV, dt = _golden_bundle(g, gr)
    _, dU = eq.tangent_bundle_step(u, dV, dt, steps=3)
    _against_golden(dU, g[f"scheme_{scheme}_classic_rk4_3"], f"{scheme}: 3 RK4 steps")


# ----------------------------------------------------------------------------- 2. the bits of tangent_step
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_every_member_has_the_bits_of_tangent_step(scheme, n, dtype):
    ph = S.Physics(scheme, n, wave=4 if n > 8 else 2)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _to(_smooth(n), dtype)
    members = [_to(m, dtype) for m in _members(n, max(KS))]
    _check_bits_of_tangent_step(eq, u, members, dt, f"{scheme} n={n} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 80])
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_bits_of_tangent_step_at_the_limiter_ties(scheme, n, dtype):
    """Small-integer states: face velocities and differences that are exactly zero, in either precision."""
    ph = S.Physics(scheme, n)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    members = [_to(m, dtype) for m in _members(n, max(KS), seed=1)]
    for name in F.EDGE_STARTS:
        u = _pair(torch.stack([F.degenerate_start(name, n, seed=n + s) for s in range(B)]), dtype)
        _check_bits_of_tangent_step(eq, u, members, dt, f"{name} {scheme} n={n} {dtype}")


@pytest.mark.parametrize("case", list(F.OPTIONAL_TERMS) + list(F.TABLEAUX))
def test_bits_of_tangent_step_with_optional_terms_and_general_tableaux(case):
    """No drag, no forcing, a dense set of terms, a negative drag; tableaux with two earlier stages feeding one stage state,
    negative weights and a zero row.  n = 80 x 3."""
    import torch_cfd_amd as tc

    e = load_golden("fvm_edges.npz")
    if case in F.TABLEAUX:
        ph, solver = F.Physics.of_golden(e, "a3", n=80), tc.RKStepper(tableau=F.TABLEAUX[case], dtype=torch.float64)
    else:
        ph, solver = F.Physics.of_golden(e, f"a2_{case}", n=80), _stepper()
    eq, dt = ph.equation(solver), 0.25 * ph.h
    _check_bits_of_tangent_step(eq, _smooth(80), _members(80, max(KS), seed=2), dt, case)


# ----------------------------------------------------------------------------- 3. the state half, steps = 0, chaining, two runs
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_state_bits_chaining_and_determinism(scheme):
    n, K = 80, 3
    ph = S.Physics(scheme, n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u, dV = _smooth(n), _bundle(_members(n, K, seed=3))
    out, dU = eq.tangent_bundle_step(u, dV, dt, steps=3)
    assert _equal(out, eq(u, dt, steps=3))
    again = eq.tangent_bundle_step(u, dV, dt, steps=3)
    assert _equal(out, again[0]) and _equal(dU, again[1])
    k, dK = eq.explicit_terms_jvp_bundle(u, dV, dt)
    again = eq.explicit_terms_jvp_bundle(u, dV, dt)
    assert _equal(k, again[0]) and _equal(dK, again[1])
    same, dsame = eq.tangent_bundle_step(u, dV, dt, steps=0)
    assert _equal(same, u) and _equal(dsame, dV)
    cu, cdV = u, dV
    for _ in range(3):
        cu, cdV = eq.tangent_bundle_step(cu, cdV, dt)
    assert _equal(out, cu) and _equal(dU, cdV)
    # a single (n, n) state: the bundle components are (K, n, n)
    one, dOne = eq.tangent_bundle_step(tuple(c[1] for c in u), tuple(c[:, 1] for c in dV), dt, steps=3)
    assert dOne[0].shape == (K, n, n)
    assert _equal(one, tuple(c[1] for c in out)) and _equal(dOne, tuple(c[:, 1] for c in dU))
    # the plans of the plain and of the pair calls never become bundle plans
    assert all(p.bundle == K for per_k in eq._bundle_plans.values() for p in per_k.values())
    assert not any(p.bundle for p in list(eq._plans.values()) + list(eq._tangent_plans.values()))


# ----------------------------------------------------------------------------- 4. members are independent
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["van_leer", "upwind"])
def test_a_member_keeps_its_bits_whatever_the_others_hold(scheme, dtype):
    n, K = 80, 5
    ph = S.Physics(scheme, n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _to(_smooth(n), dtype)
    dV = _bundle([_to(m, dtype) for m in _members(n, K, seed=4)])
    out, dU = eq.tangent_bundle_step(u, dV, dt, steps=3)
    k, dK = eq.explicit_terms_jvp_bundle(u, dV, dt)
    for keep in (0, 2, K - 1):
        bad = tuple(c.clone() for c in dV)
        for m, fill in zip([m for m in range(K) if m != keep], (float("nan"), float("inf"), float("-inf"), float("nan"))):
            for c in bad:
                c[m].fill_(fill)
        out2, dU2 = eq.tangent_bundle_step(u, bad, dt, steps=3)
        k2, dK2 = eq.explicit_terms_jvp_bundle(u, bad, dt)
        assert _equal(out, out2) and _equal(k, k2), keep
        assert _equal(_member(dU, keep), _member(dU2, keep)) and _equal(_member(dK, keep), _member(dK2, keep)), keep


# ----------------------------------------------------------------------------- 5. ensembles
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_bundle_on_an_ensemble_is_the_scalar_operator_per_member(scheme, dtype):
    """B = 3 members, drag on one only, forcing scale one: field b and its tangents have the bits of the scalar operator
    (nu_b, drag_b) on field b alone with the same tangents."""
    import torch_cfd_amd as tc

    n, K = 80, 3
    nu, drag = (1e-2, 3e-3, 1e-3), (0.0, 0.2, 0.0)
    ph = S.Physics(scheme, n, wave=2)
    grid = ph.grid()

    def equation(v, d, fs=None):
        forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=2, offsets=grid.cell_faces)
        return tc.NavierStokes2DFVMProjection(v, grid, drag=d, forcing=forcing, solver=_stepper(), convect=ph.descriptor(),
                                              forcing_scale=fs)

    dt = 0.25 * ph.h
    u = _to(_smooth(n), dtype)
    members = [_to(m, dtype) for m in _members(n, K, seed=5)]
    dV = _bundle(members)
    ens = equation(list(nu), list(drag), [1.0] * B)
    out, dU = ens.tangent_bundle_step(u, dV, dt, steps=3)
    k, dK = ens.explicit_terms_jvp_bundle(u, dV, dt)
    for m in range(K):   # against the ensemble's own pair calls
        assert _equal(_member(dU, m), ens.tangent_step(u, members[m], dt, steps=3)[1]), m
    for b in range(B):
        one = equation(nu[b], drag[b])
        ub, dVb = tuple(c[b:b + 1] for c in u), tuple(c[:, b:b + 1] for c in dV)
        o1, d1 = one.tangent_bundle_step(ub, dVb, dt, steps=3)
        assert _equal(tuple(c[b:b + 1] for c in out), o1) and _equal(tuple(c[:, b:b + 1] for c in dU), d1), ("step", b)
        k1, dk1 = one.explicit_terms_jvp_bundle(ub, dVb, dt)
        assert _equal(tuple(c[b:b + 1] for c in k), k1) and _equal(tuple(c[:, b:b + 1] for c in dK), dk1), ("explicit terms", b)
    assert not torch.equal(dU[0][0, 0], equation(nu[1], drag[1]).tangent_bundle_step(u, dV, dt, steps=3)[1][0][0, 0])


# ----------------------------------------------------------------------------- 6. adjoint identity with the existing VJP
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_adjoint_identity_of_every_member_against_the_vjp_kernels(scheme):
    """<J dU_k, g> = <dU_k, J^T g>, the bound of test_adjoint_identity_against_the_vjp_kernels: each side may be off by
    FP64_BOUND relative to its own factors."""
    n, K = 32, 3
    ph = S.Physics(scheme, n, wave=4)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    u = _smooth(n, 2)
    members = _members(n, K, batch=2, seed=6)
    dV = _bundle(members)
    g = J.perturbation((2, 2, n, n), 5 * n, DEV)
    dot = lambda p, q: sum((x * y).sum() for x, y in zip(p, q)).item()
    norm = lambda p: math.sqrt(dot(p, p))
    for what, bundle, fn in (("explicit terms", eq.explicit_terms_jvp_bundle(u, dV, dt)[1], lambda w: eq.explicit_terms(w, dt)),
                             ("3 steps", eq.tangent_bundle_step(u, dV, dt, steps=3)[1], lambda w: eq(w, dt, steps=3))):
        leaves = tuple(c.clone().requires_grad_() for c in u)
        jtg = torch.autograd.grad(sum((o * c).sum() for o, c in zip(fn(leaves), g)), leaves)
        for k in range(K):
            jv, v = _member(bundle, k), members[k]
            lhs, rhs = dot(jv, g), dot(v, jtg)
            bound = FP64_BOUND * (norm(jv) * norm(g) + norm(v) * norm(jtg))
            print(f"{scheme} {what} member {k}: <Jv, g> {lhs:.12e}, <v, J^T g> {rhs:.12e}, bound {bound:.2e}")
            assert abs(lhs - rhs) <= bound, (what, k, lhs, rhs)


# ----------------------------------------------------------------------------- 7. refusals of the C ABI
def test_refusals_of_the_c_abi_leave_the_outputs_untouched():
    import torch_cfd_amd as tc
    from torch_cfd_amd import _lib

    lib = _lib.load()
    n, K = 16, 2
    ph = F.Physics(n)
    eq, dt = ph.equation(_stepper()), 0.25 * ph.h
    bundle, tangent, plain = eq._bundle_plan(torch.float64, DEV, K), eq._plan(torch.float64, DEV, tangent=True), eq._plan(torch.float64, DEV)
    a, b = eq.solver.weights(dt)
    ca, cb = _lib.darray(a), _lib.darray(b)
    ux, uy = (c.contiguous() for c in _smooth(n, 6))
    gx, gy = J.perturbation((6, 2, n, n), 2, DEV)
    ox, oy = torch.full_like(ux, 7.0), torch.full_like(uy, 7.0)
    ws = bundle.workspace(6, lib.tcfd_fvm_step_vjp_workspace_bytes(bundle.handle, 6))
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    P = lambda t: t.data_ptr()
    h = bundle.handle

    def refused(rc, word):
        torch.cuda.synchronize()
        msg = lib.tcfd_last_error().decode()
        assert rc == TCFD_EINVAL and word in msg, (rc, msg)
        assert bool((ox == 7.0).all()) and bool((oy == 7.0).all())

    with torch.cuda.device(torch.device(DEV)):
        refused(lib.tcfd_fvm_plan_set_tangent_bundle(None, 2), "null plan")
        refused(lib.tcfd_fvm_plan_set_tangent_bundle(plain.handle, -1), "ntangents = -1")
        refused(lib.tcfd_fvm_plan_set_tangent_bundle(plain.handle, _lib.TCFD_FVM_MAX_TANGENTS + 1), "outside")
        # the bundle and the tangent setting exclude each other; the refused call leaves the plan as it was
        refused(lib.tcfd_fvm_plan_set_tangent_bundle(tangent.handle, 2), "tangent plan")
        refused(lib.tcfd_fvm_plan_set_tangent(h, 1), "bundle plan")
        refused(lib.tcfd_fvm_explicit_terms(tangent.handle, P(ux), P(uy), P(ox), P(oy), 3, dt, stream), "pairs")
        # a batch that is no multiple of 1 + K
        refused(lib.tcfd_fvm_explicit_terms(h, P(ux), P(uy), P(ox), P(oy), 4, dt, stream), "whole bundles")
        refused(lib.tcfd_fvm_step(h, P(ux), P(uy), P(ox), P(oy), 5, 1, len(b), ca, cb, dt, P(ws), ws.numel(), stream), "whole bundles")
        # more fields than the launch grids take: refused before anything is read
        big = 3 * 21846
        refused(lib.tcfd_fvm_explicit_terms(h, P(ux), P(uy), P(ox), P(oy), big, dt, stream), "launch grids")
        refused(lib.tcfd_fvm_step(h, P(ux), P(uy), P(ox), P(oy), big, 1, len(b), ca, cb, dt, P(ws), ws.numel(), stream), "launch grids")
        # reverse mode on a bundle plan
        refused(lib.tcfd_fvm_explicit_terms_vjp(h, P(ux), P(uy), P(gx), P(gy), P(ox), P(oy), 6, dt, stream), "bundle plan")
        saved = torch.stack([ux, uy])[None].contiguous()
        refused(lib.tcfd_fvm_step_vjp(h, P(saved), P(gx), P(gy), P(ox), P(oy), 6, 1, len(b), ca, cb, dt, P(ws), ws.numel(), stream),
                "bundle plan")
        # an ensemble of 2 members on a bundle plan of K = 2 takes 6 fields, not 3
        ens = tc.NavierStokes2DFVMProjection([1e-3, 2e-3], ph.grid(), drag=[0.1, 0.0], solver=_stepper())
        he = ens._bundle_plan(torch.float64, DEV, K).handle
        refused(lib.tcfd_fvm_explicit_terms(he, P(ux), P(uy), P(ox), P(oy), 3, dt, stream), "per-sample parameters")
        refused(lib.tcfd_fvm_step(he, P(ux), P(uy), P(ox), P(oy), 9, 1, len(b), ca, cb, dt, P(ws), ws.numel(), stream),
                "per-sample parameters")
        # the bundle plan is still one of K = 2, and clearing it makes a plain plan again
        assert lib.tcfd_fvm_explicit_terms(h, P(ux), P(uy), P(ox), P(oy), 6, dt, stream) == 0
        torch.cuda.synchronize()
        (kx, ky), (dkx, dky) = eq.explicit_terms_jvp_bundle((ux[:2], uy[:2]), (ux[2:].reshape(2, 2, n, n), uy[2:].reshape(2, 2, n, n)), dt)
        assert torch.equal(ox, torch.cat([kx, dkx.reshape(4, n, n)])) and torch.equal(oy, torch.cat([ky, dky.reshape(4, n, n)]))
        fresh = tc.NavierStokes2DFVMProjection(ph.nu, ph.grid(), drag=ph.drag, solver=_stepper())._bundle_plan(torch.float64, DEV, K)
        assert lib.tcfd_fvm_plan_set_tangent_bundle(fresh.handle, 0) == 0
        assert lib.tcfd_fvm_explicit_terms(fresh.handle, P(ux), P(uy), P(ox), P(oy), 5, dt, stream) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 8. memory contract of the bundle plan
def _guard(what, ins, outs, call, need, baseline):
    """One guarded case by the protocol of tests/guard_ops.py (as tests/test_fvm_jvp_gpu.py runs it)."""
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_memory_contract_of_the_bundle_plan(dtype):
    """tcfd_fvm_explicit_terms and tcfd_fvm_step on a bundle plan, K = 2, B = 2, n = 16: inputs unchanged, nothing outside the
    outputs and the declared workspace written, results independent of what the scratch held, bit-equal to the wrapper path; a
    workspace one byte short is TCFD_EWORKSPACE and touches no output (run_guarded's last call)."""
    import torch_cfd_amd as tc
    from torch_cfd_amd import _lib

    lib = _lib.load()
    n, K, fields = 16, 2, 6
    ph = F.Physics(n)
    solver = tc.RKStepper(tableau=F.TABLEAUX["ssprk3"], dtype=torch.float64)
    eq, dt = ph.equation(solver), 0.25 * ph.h
    plan = eq._bundle_plan(dtype, DEV, K)
    a, b = solver.weights(dt)
    ca, cb = _lib.darray(a), _lib.darray(b)
    u = _smooth(n, 2)
    dV = _bundle(_members(n, K, batch=2, seed=8))
    ux, uy = (torch.cat([s, d.reshape(-1, n, n)]).to(dtype).contiguous() for s, d in zip(u, dV))
    o = Out(dtype, (fields, n, n))
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    h = plan.handle
    kx, ky = plan.explicit_terms(ux, uy, dt)
    _guard("tcfd_fvm_explicit_terms on a bundle plan", {"ux": ux, "uy": uy}, {"kx": o, "ky": o},
           lambda P, ws, nb: lib.tcfd_fvm_explicit_terms(h, P("ux"), P("uy"), P("kx"), P("ky"), fields, dt, stream()),
           None, {"kx": kx, "ky": ky})
    need = lib.tcfd_fvm_workspace_bytes(h, fields)
    assert need == lib.tcfd_fvm_workspace_bytes(eq._plan(dtype, DEV).handle, fields)   # the carve for (1 + K) B holds all of it
    sx, sy = plan.step(ux, uy, dt, a, b, 2)
    _guard("tcfd_fvm_step on a bundle plan", {"ux": ux, "uy": uy}, {"ox": o, "oy": o},
           lambda P, ws, nb: lib.tcfd_fvm_step(h, P("ux"), P("uy"), P("ox"), P("oy"), fields, 2, 3, ca, cb, dt, ws, nb, stream()),
           need, {"ox": sx, "oy": sy})
    # one byte short, said directly as well
    ws = plan.workspace(fields)
    ox, oy = torch.full_like(ux, 7.0), torch.full_like(uy, 7.0)
    with torch.cuda.device(torch.device(DEV)):
        rc = lib.tcfd_fvm_step(h, ux.data_ptr(), uy.data_ptr(), ox.data_ptr(), oy.data_ptr(), fields, 2, 3, ca, cb, dt,
                               ws.data_ptr(), need - 1, stream())
    torch.cuda.synchronize()
    assert rc == TCFD_EWORKSPACE and bool((ox == 7.0).all()) and bool((oy == 7.0).all())
