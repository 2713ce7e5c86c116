"""GPU tests of finite-volume ensembles: per-sample viscosity, drag and forcing amplitude on the EnsConst instantiations of
k_fvm_stage, k_fvm_stage_jvp and k_fvm_stage_vjp (tcfd_fvm.hip, tcfd_fvm_plan_set_ensemble) through
``NavierStokes2DFVMProjection(viscosity=[...], drag=[...], forcing_scale=[...])``.

Sizes: n = 16 (one partly masked 64 x 4 block along x) and n = 80 (a full block and a partly masked one along x, 20 blocks along
y).  An odd size such as 31 cannot be built: the pressure solve's rfft pseudo-inverse refuses odd grids and the transform plan
takes n = 2^k, 3 * 2^k >= 96 and 5 * 2^k >= 80 only, all multiples of four, so no size this solver runs leaves a partial block
along y; n = 80 is the smallest size with more than one block along x and a masked tail.  B = 5 members, one without drag beside
members with drag.  The solver does not split a batch, so there is no chunk boundary to span.

Bounds: the golden comparison uses the bounds of tests/test_fvm_gpu.py for its step goldens (fp64 1e-11, fp32 1e-5) and the
tangent bound of tests/test_fvm_jvp_gpu.py (1e-10); the dot-product identity uses that file's bound for the scalar operator."""
import ctypes
import math

import pytest
import torch
import torch.autograd.forward_ad as fwAD

import fvm_jvp_ops as J
import fvm_schemes_ops as S
from conftest import load_golden, rel_l2
from guard_ops import Arena, Out, nbytes, run_guarded

pytestmark = pytest.mark.gpu
L = 2 * math.pi
DEV = "cuda:0"
FP64_BOUND = 1e-10                      # tests/test_fvm_jvp_gpu.py
STEP_BOUND = {torch.float64: 1e-11, torch.float32: 1e-5}     # tests/test_fvm_gpu.py, its step goldens
SIZES = (16, 80)
DTYPES = (torch.float64, torch.float32)
NU = (1e-2, 3e-3, 1e-3, 3e-4, 5e-3)
DRAG = (0.1, 0.0, 0.2, 0.05, 0.0)       # members 1 and 4 have no drag
B = len(NU)
TCFD_EINVAL = -1


@pytest.fixture(autouse=True)
def fp64_default():
    """The grid and the forcing table are formed in the default dtype: fp64, as the reference's runs of the goldens (the fields
    of a test carry their own dtype)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _equation(n, scheme, nu, drag, forcing_scale=None, forced=True, method="classic_rk4", solver=None):
    import torch_cfd_amd as tc

    ph = S.Physics(scheme, n, wave=2)
    grid = ph.grid()
    forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=2, offsets=grid.cell_faces) if forced else None
    solver = tc.RKStepper.from_method(method=method) if solver is None else solver
    return tc.NavierStokes2DFVMProjection(nu, grid, drag=drag, forcing=forcing, solver=solver, convect=ph.descriptor(),
                                          forcing_scale=forcing_scale)


_STARTS = {}


def _start(n, dtype, batch=B):
    """A smooth (batch, n, n) velocity pair and a seeded perturbation and cotangent of it, made once per size."""
    if (n, batch) not in _STARTS:
        from torch_cfd_amd import initial_conditions as ic

        ph = S.Physics("van_leer", n)
        ux, uy = ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=DEV, batch_seeds=list(range(batch)))
        u = (ux.detach().double().clone(), uy.detach().double().clone())
        _STARTS[(n, batch)] = (u, J.perturbation((batch, 2, n, n), 7 * n, DEV), J.perturbation((batch, 2, n, n), 11 * n, DEV))
    return tuple(tuple(c.to(dtype) for c in p) for p in _STARTS[(n, batch)])


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _member(p, b):
    return tuple(c[b:b + 1] for c in p)


def _grad(eq, u, g, dt, steps):
    """Gradient with respect to u0 of the quadratic loss sum(0.5 g out^2)."""
    leaves = tuple(c.clone().requires_grad_() for c in u)
    out = eq(leaves, dt, steps=steps)
    loss = sum((0.5 * w * o * o).sum() for o, w in zip(out, g))
    return torch.autograd.grad(loss, leaves)


# ----------------------------------------------------------------------------- 1. bitwise: member b is the scalar operator
@pytest.mark.parametrize("scheme", S.SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_member_b_is_bit_equal_to_the_scalar_operator_of_its_values(n, dtype, scheme):
    """Stepping, the explicit terms, the tangent-linear step (state and tangent) and the gradient with respect to u0; forcing
    scale one.  A member without drag sits beside members with drag."""
    dt = 0.25 * L / n
    u, du, g = _start(n, dtype)
    ens = _equation(n, scheme, list(NU), list(DRAG), forcing_scale=[1.0] * B)
    out = ens(u, dt, steps=3)
    k = ens.explicit_terms(u, dt)
    ts, tt = ens.tangent_step(u, du, dt, steps=2)
    ks, kt = ens.explicit_terms_jvp(u, du, dt)
    gr = _grad(ens, u, g, dt, 2)
    assert out[0].shape == (B, n, n) and out[0].dtype == dtype
    for b in range(B):
        one = _equation(n, scheme, NU[b], DRAG[b])
        ub, dub, gb = _member(u, b), _member(du, b), _member(g, b)
        assert _equal(_member(out, b), one(ub, dt, steps=3)), ("step", b)
        assert _equal(_member(k, b), one.explicit_terms(ub, dt)), ("explicit terms", b)
        s1, t1 = one.tangent_step(ub, dub, dt, steps=2)
        assert _equal(_member(ts, b), s1) and _equal(_member(tt, b), t1), ("tangent step", b)
        s1, t1 = one.explicit_terms_jvp(ub, dub, dt)
        assert _equal(_member(ks, b), s1) and _equal(_member(kt, b), t1), ("explicit terms jvp", b)
        assert _equal(_member(gr, b), _grad(one, ub, gb, dt, 2)), ("gradient", b)
    # the members differ: the result is no broadcast of one member's physics
    same = _equation(n, scheme, NU[0], DRAG[0])(u, dt, steps=3)
    assert not any(torch.equal(same[0][b], out[0][b]) for b in range(1, B))


# ----------------------------------------------------------------------------- 2. the reference's own runs, forcing scales included
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_stacked_scalar_runs_of_the_reference(dtype):
    g = load_golden("fvm_ensemble.npz")
    n, dt = int(g["n"]), float(g["dt"])
    eq = _equation(n, "van_leer", g["nu"].tolist(), g["drag"].tolist(), forcing_scale=g["scale"].tolist())
    u0 = J.pair(g["u0"], DEV, dtype)
    for steps in (1, 5):
        err = rel_l2(J.stacked(eq(u0, dt, steps=steps)), g[f"steps_{steps}"])
        print(f"{dtype} {steps} steps: rel-L2 {err:.2e}, bound {STEP_BOUND[dtype]:.0e}")
        assert err <= STEP_BOUND[dtype], (steps, err)
    if dtype == torch.float64:
        assert STEP_BOUND[dtype] == float(g["tolerance"])        # the bound the generator measured its margins against
        _, du = eq.tangent_step(u0, J.pair(g["du"], DEV, dtype), dt)
        err = rel_l2(J.stacked(du), g["tangent_1"])
        print(f"tangent of one step: rel-L2 {err:.2e}")
        assert err <= FP64_BOUND, err


# ----------------------------------------------------------------------------- 3. dot-product identity on the ensemble
@pytest.mark.parametrize("scheme", S.SCHEMES)
@pytest.mark.parametrize("n", SIZES)
def test_dot_product_identity_between_the_tangent_and_the_adjoint(n, scheme):
    """<J dv, g> = <dv, J^T g>: k_fvm_stage_jvp against k_fvm_stage_vjp, both on the member table, distinct forcing scales."""
    dt = 0.25 * L / n
    u, v, g = _start(n, torch.float64)
    eq = _equation(n, scheme, list(NU), list(DRAG), forcing_scale=[1.0, 0.5, 2.0, 0.0, -1.0])
    dot = lambda p, q: sum((x * y).sum() for x, y in zip(p, q)).item()
    norm = lambda p: math.sqrt(dot(p, p))
    for steps in (1, 2):
        jv = eq.tangent_step(u, v, dt, steps=steps)[1]
        leaves = tuple(c.clone().requires_grad_() for c in u)
        out = eq(leaves, dt, steps=steps)
        jtg = torch.autograd.grad(sum((o * c).sum() for o, c in zip(out, g)), leaves)
        lhs, rhs = dot(jv, g), dot(v, jtg)
        bound = FP64_BOUND * (norm(jv) * norm(g) + norm(v) * norm(jtg))
        print(f"{scheme} n={n} {steps} steps: <Jv, g> {lhs:.12e}, <v, J^T g> {rhs:.12e}, bound {bound:.2e}")
        assert abs(lhs - rhs) <= bound, (steps, lhs, rhs)


# ----------------------------------------------------------------------------- 4. plumbing
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_steps_trajectories_permutations_and_reruns_agree_bit_for_bit(n, dtype):
    import torch_cfd_amd as tc

    dt = 0.25 * L / n
    u, du, _ = _start(n, dtype)
    fs = [1.0, 0.5, 2.0, 0.0, -1.0]
    eq = _equation(n, "van_leer", list(NU), list(DRAG), forcing_scale=fs)
    out = eq(u, dt, steps=4)
    assert _equal(out, eq(u, dt, steps=4)) and _equal(out, eq.advance(u, dt, steps=4))       # run to run
    chained = u
    for _ in range(4):
        chained = eq.solver(chained, dt, eq)                                                  # RKStepper.forward, one step
    assert _equal(out, chained)
    tx, ty = tc.get_trajectory_fvm(eq, u, dt, num_steps=4, record_every_steps=2)
    assert tx.shape == (B, 2, n, n)
    assert _equal((tx[:, 0], ty[:, 0]), eq(u, dt, steps=2)) and _equal((tx[:, 1], ty[:, 1]), out)
    # the members permuted: the result permuted
    perm = [3, 0, 4, 2, 1]
    peq = _equation(n, "van_leer", [NU[i] for i in perm], [DRAG[i] for i in perm], forcing_scale=[fs[i] for i in perm])
    pout = peq(tuple(c[perm].contiguous() for c in u), dt, steps=4)
    assert _equal(pout, tuple(c[perm] for c in out))
    # every other tableau takes the members too; the tangent plan's state half is the plain plan's result
    for method in ("forward_euler", "midpoint", "heun_rk2"):
        solver = tc.RKStepper.from_method(method=method)
        ens = _equation(n, "van_leer", list(NU), list(DRAG), forcing_scale=fs, solver=solver)
        got = solver(u, dt, ens)
        for b in (1, 2):
            one = _equation(n, "van_leer", NU[b], DRAG[b], forcing_scale=fs[b], solver=solver)
            err = rel_l2(J.stacked(_member(got, b)), J.stacked(solver(_member(u, b), dt, one)))
            assert err <= 10 * torch.finfo(dtype).eps, (method, b, err)      # fl(s f) against a table of s f: roundings apart
    ts, tt = eq.tangent_step(u, du, dt, steps=4)
    assert _equal(ts, out)
    with fwAD.dual_level():      # dual numbers run the same calls
        parts = [fwAD.unpack_dual(o) for o in eq(tuple(fwAD.make_dual(a, t) for a, t in zip(u, du)), dt, steps=4)]
        assert _equal(tuple(p.primal for p in parts), ts) and _equal(tuple(p.tangent for p in parts), tt)
    # a member table that changes in place builds a new plan
    plan = eq._plan(dtype, torch.device(DEV))
    eq.drag[1] = 0.3
    assert eq._plan(dtype, torch.device(DEV)) is not plan
    moved = eq(u, dt, steps=4)
    assert not torch.equal(moved[0][1], out[0][1]) and torch.equal(moved[0][0], out[0][0])


def test_refusals_of_the_python_entry_points():
    n, dt = 16, 0.25 * L / 16
    u, du, g = _start(n, torch.float64)
    eq = _equation(n, "van_leer", list(NU), list(DRAG))
    for bad in (tuple(c[:3] for c in u), tuple(c[0] for c in u)):
        with pytest.raises(ValueError, match=f"B = {B}"):
            eq(bad, dt)
        with pytest.raises(ValueError, match=f"B = {B}"):
            eq.tangent_step(bad, bad, dt)
    leaves = tuple(c.clone().requires_grad_() for c in u)
    out = eq(leaves, dt, steps=2)
    with pytest.raises(NotImplementedError, match="double backward"):       # the adjoint kernels are first order
        torch.autograd.grad(sum((o * o).sum() for o in out), leaves, create_graph=True)
    k = eq.explicit_terms(leaves, dt)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(sum((o * o).sum() for o in k), leaves, create_graph=True)
    eq.viscosity.requires_grad_()
    with pytest.raises(NotImplementedError, match="requires grad"):
        eq(u, dt)


# ----------------------------------------------------------------------------- 5. the scalar path of a plan is untouched
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_plan_is_scalar_again_after_its_table_is_cleared_and_refusals_leave_it_usable(dtype):
    from torch_cfd_amd import _lib

    lib = _lib.load()
    n, dt = 16, 0.25 * L / 16
    u, _, _ = _start(n, dtype)
    scalar = _equation(n, "van_leer", NU[0], DRAG[0])
    ens = _equation(n, "van_leer", list(NU), list(DRAG), forcing_scale=[1.0, 0.5, 2.0, 0.0, -1.0])
    a, b = scalar.solver.weights(dt)
    plan = scalar._plan(dtype, torch.device(DEV))
    first = plan.step(*u, dt, a, b, 3)
    plan.set_ensemble(list(NU), list(DRAG), [1.0, 0.5, 2.0, 0.0, -1.0])
    assert plan.members == B
    assert _equal(plan.step(*u, dt, a, b, 3), ens(u, dt, steps=3))
    # refused calls: a batch other than the members (both numbers named), bad arguments; the table stays as it was
    with pytest.raises(_lib.TcfdError, match=rf"batch 3 .* {B} fields"):
        plan.step(u[0][:3], u[1][:3], dt, a, b, 3)
    with pytest.raises(_lib.TcfdError, match=rf"batch 3 .* {B} fields"):
        plan.explicit_terms(u[0][:3], u[1][:3], dt)
    with pytest.raises(_lib.TcfdError, match=rf"batch 3 .* {B} fields"):
        plan.explicit_terms_vjp(u[0][:3], u[1][:3], u[0][:3], u[1][:3], dt)
    nu = _lib.darray(NU)
    assert lib.tcfd_fvm_plan_set_ensemble(plan.handle, -1, nu, None, None) == TCFD_EINVAL and b"count -1" in lib.tcfd_last_error()
    assert lib.tcfd_fvm_plan_set_ensemble(plan.handle, B, None, None, None) == TCFD_EINVAL and b"required" in lib.tcfd_last_error()
    assert _equal(plan.step(*u, dt, a, b, 3), ens(u, dt, steps=3))
    tangent = scalar._plan(dtype, torch.device(DEV), tangent=True)
    tangent.set_ensemble(list(NU), list(DRAG), None)
    with pytest.raises(_lib.TcfdError, match=rf"batch 6 .* {B} members"):
        tangent.step(torch.cat([u[0][:3]] * 2), torch.cat([u[1][:3]] * 2), dt, a, b, 1)
    unforced = _equation(n, "van_leer", NU[0], DRAG[0], forced=False)
    bare, two = unforced._plan(dtype, torch.device(DEV)), tuple(c[:2] for c in u)
    want = bare.step(*two, dt, a, b, 1)
    with pytest.raises(_lib.TcfdError, match="without forcing"):
        bare.set_ensemble(list(NU), None, [1.0] * B)
    assert bare.members == 0 and _equal(bare.step(*two, dt, a, b, 1), want)
    # drag = NULL: every member takes the plan's scalar drag
    plan.set_ensemble(list(NU), None, None)
    assert _equal(plan.step(*u, dt, a, b, 3), _equation(n, "van_leer", list(NU), DRAG[0])(u, dt, steps=3))
    # count = 0: the scalar plan again, any batch, the bits it had
    plan.set_ensemble()
    assert plan.members == 0
    assert _equal(plan.step(*u, dt, a, b, 3), first)
    assert _equal(plan.step(u[0][:3], u[1][:3], dt, a, b, 3), tuple(c[:3] for c in first))


# ----------------------------------------------------------------------------- 6. memory contract of the ensemble calls
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
def test_memory_contract_of_the_ensemble_calls(dtype):
    """tcfd_fvm_step on an ensemble plan and on an ensemble tangent plan, tcfd_fvm_step_vjp on an ensemble plan, n = 16, B = 5:
    inputs unchanged, nothing outside the outputs and the workspace written, results independent of what the scratch held and
    bit-equal to the wrapper path; a short workspace returns TCFD_EWORKSPACE without touching an output."""
    from torch_cfd_amd import _lib

    lib = _lib.load()
    n, dt = 16, 0.25 * L / 16
    u, du, g = _start(n, dtype)
    eq = _equation(n, "van_leer", list(NU), list(DRAG), forcing_scale=[1.0, 0.5, 2.0, 0.0, -1.0])
    a, b = eq.solver.weights(dt)
    ca, cb, S4 = _lib.darray(a), _lib.darray(b), len(b)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    plan, tangent = eq._plan(dtype, torch.device(DEV)), eq._plan(dtype, torch.device(DEV), tangent=True)
    ux, uy = (c.contiguous() for c in u)
    o = Out(dtype, (B, n, n))
    h = plan.handle
    sx, sy = plan.step(ux, uy, dt, a, b, 2)
    need = lib.tcfd_fvm_workspace_bytes(h, B)
    _guard("tcfd_fvm_step on an ensemble plan", {"ux": ux, "uy": uy}, {"ox": o, "oy": o},
           lambda P, ws, nb: lib.tcfd_fvm_step(h, P("ux"), P("uy"), P("ox"), P("oy"), B, 2, S4, ca, cb, dt, ws, nb, stream()),
           need, {"ox": sx, "oy": sy})
    kx, ky = plan.explicit_terms(ux, uy, dt)
    _guard("tcfd_fvm_explicit_terms on an ensemble plan", {"ux": ux, "uy": uy}, {"kx": o, "ky": o},
           lambda P, ws, nb: lib.tcfd_fvm_explicit_terms(h, P("ux"), P("uy"), P("kx"), P("ky"), B, dt, stream()),
           None, {"kx": kx, "ky": ky})
    # the tangent plan: pairs, 2 B fields
    px, py = (torch.cat([s, d]).contiguous() for s, d in zip(u, du))
    o2 = Out(dtype, (2 * B, n, n))
    ht = tangent.handle
    tx, ty = tangent.step(px, py, dt, a, b, 2)
    _guard("tcfd_fvm_step on an ensemble tangent plan", {"ux": px, "uy": py}, {"ox": o2, "oy": o2},
           lambda P, ws, nb: lib.tcfd_fvm_step(ht, P("ux"), P("uy"), P("ox"), P("oy"), 2 * B, 2, S4, ca, cb, dt, ws, nb, stream()),
           lib.tcfd_fvm_workspace_bytes(ht, 2 * B), {"ox": tx, "oy": ty})
    # the reverse of two steps
    saved, _, _ = plan.step_saving(ux, uy, dt, a, b, 2)
    gx, gy = (c.contiguous() for c in g)
    bx, by = plan.step_vjp(saved, gx, gy, dt, a, b)
    _guard("tcfd_fvm_step_vjp on an ensemble plan", {"saved": saved, "gx": gx, "gy": gy}, {"ox": o, "oy": o},
           lambda P, ws, nb: lib.tcfd_fvm_step_vjp(h, P("saved"), P("gx"), P("gy"), P("ox"), P("oy"), B, 2, S4, ca, cb, dt, ws, nb,
                                                   stream()),
           lib.tcfd_fvm_step_vjp_workspace_bytes(h, B), {"ox": bx, "oy": by})
