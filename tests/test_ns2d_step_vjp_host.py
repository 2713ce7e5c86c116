"""Host-side checks of the adjoint model of the spectral step (no GPU): the golden gradients made from the reference
(tests/golden/ns2d_step_vjp.npz) against the CPU oracle and the plain-torch restatement under torch.autograd, the reverse sweep of
include/tcfd_ns2d_adjoint.h (tcfd_ns2d_step_vjp) written out in torch against autograd, the new names of the ABI and of the operator, and the
argument checks that run before any device call."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ns2d_ops  # noqa: E402
import ns2d_step_vjp_ops as V  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402

L = 2 * math.pi


def _golden(prefix=""):
    g = load_golden("ns2d_step_vjp.npz")
    return g, torch.from_numpy(g[prefix + "w0"]), torch.from_numpy(g[prefix + "cot"]), float(g["dt"])


def _grad(fn, w0, cot):
    w = w0.clone().requires_grad_(True)
    ns2d_ops.real_inner(cot, fn(w)).backward()
    return w.grad


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", ["none", "kolmogorov"])
def test_oracle_and_restatement_gradients_match_the_reference(forcing, smooth):
    """oracle/ns2d.py under autograd against the reference's own gradients for RK4-CN at 1 and 3 steps, and the stage loop of
    tests/ns2d_ops.py on the package's schedules for the three IMEX orders at 2 steps (fp64, n = 16, B = 2).  Bound: 1e-12 --
    the same fp64 torch ops up to association."""
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float64)
    g, w0, cot, dt = _golden()
    t = ns2d_ops.tables(16, forcing, smooth)
    key = f"{forcing}_s{int(smooth)}_"
    for what, (solver, steps) in V.GOLDEN_RUNS.items():
        sched = ns2d_ops.schedule(V.make_solver(solver), dt)
        got = _grad(lambda w: ns2d_ops.advance(w, t, sched, steps), w0, cot)
        assert rel_l2(got, g[key + what]) <= 1e-12, what
        if solver == "rk4":
            got = _grad(lambda w: O.advance(w, dt, t.oracle, steps=steps)[0], w0, cot)
            assert rel_l2(got, g[key + what]) <= 1e-12, what


def test_oracle_gradient_in_single_precision():
    """The complex64 golden (a float32 run of the reference).  Bound 2e-5, the project's fp32 bound."""
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float32)
    g, w0, cot, dt = _golden("f32_")
    assert w0.dtype == torch.complex64
    t = ns2d_ops.tables(16, "kolmogorov", True, real=torch.float32)
    got = _grad(lambda w: O.advance(w, dt, t.oracle, steps=3)[0], w0, cot)
    assert got.dtype == torch.complex64 and rel_l2(got, g["f32_kolmogorov_s1_rk3"]) <= 2e-5
    sched = ns2d_ops.schedule(V.make_solver("imex2"), dt)
    assert rel_l2(_grad(lambda w: ns2d_ops.advance(w, t, sched, 2), w0, cot), g["f32_kolmogorov_s1_imex2"]) <= 2e-5


def _reverse_sweep(saved, g_out, t, sched):
    """The reverse sweep of tcfd_ns2d_step_vjp as include/tcfd_ns2d_adjoint.h states it, in torch: stage states recomputed from each step's
    saved input, then G = hbar + gdt r ubar, fbar = fa G, hbar <- beta G, bbar = (1 + mu L) r ubar, ubar <- J_F(u_k)^T fbar +
    (base0 ? 0 : bbar), ubar_start += base0 ? bbar : 0.  J_F^T by autograd of the explicit terms alone."""
    n = len(sched["beta"])
    fa = sched.get("fa") or [1.0] * n
    mud = sched.get("mu_den") or sched["mu"]
    base0 = sched.get("base0") or [0] * n
    lin = t.linear_term
    ubar = g_out
    for u0 in reversed(saved):
        states, u, h = [u0], u0, None
        for k in range(n - 1):
            f = ns2d_ops.explicit_terms(u, t)
            h = fa[k] * f if h is None else fa[k] * f + sched["beta"][k] * h
            b = u0 if base0[k] else u
            u = (b + sched["gdt"][k] * h + sched["mu"][k] * (lin * b)) / (1 - mud[k] * lin)
            states.append(u)
        hbar, ustart = None, None
        for k in range(n - 1, -1, -1):
            r = 1 / (1 - mud[k] * lin)
            G = sched["gdt"][k] * r * ubar if hbar is None else hbar + sched["gdt"][k] * r * ubar
            hbar = sched["beta"][k] * G
            bbar = (1 + sched["mu"][k] * lin) * r * ubar
            uk = states[k].clone().requires_grad_(True)
            (jt,) = torch.autograd.grad(ns2d_ops.real_inner(fa[k] * G, ns2d_ops.explicit_terms(uk, t)), uk)
            if base0[k] and k > 0:
                ustart = bbar if ustart is None else ustart + bbar
                ubar = jt
            else:
                ubar = jt + bbar
        if ustart is not None:
            ubar = ubar + ustart
    return ubar


@pytest.mark.parametrize("solver,steps", [("rk4", 2), ("imex1.5", 2), ("imex2", 3)])
def test_the_documented_reverse_sweep_is_the_gradient(solver, steps):
    """The recurrences the header documents (and the kernels implement) reproduce the golden gradients of the reference from the
    saved step inputs alone -- including the schedule whose second stage restarts from the step's initial state."""
    torch.set_default_dtype(torch.float64)
    g, w0, cot, dt = _golden()
    t = ns2d_ops.tables(16, "kolmogorov", True)
    sched = ns2d_ops.schedule(V.make_solver(solver), dt)
    saved = [w0]
    for _ in range(steps - 1):
        saved.append(ns2d_ops.step(saved[-1], t, sched))
    got = _reverse_sweep(saved, cot, t, sched)
    want = _grad(lambda w: ns2d_ops.advance(w, t, sched, steps), w0, cot)
    assert rel_l2(got, want) <= 1e-13
    name = {("rk4", 2): None, ("imex1.5", 2): "imex1.5", ("imex2", 3): None}[(solver, steps)]
    if name:
        assert rel_l2(got, g["kolmogorov_s1_" + name]) <= 1e-12


def test_golden_is_small_and_numeric():
    from conftest import GOLDEN

    assert os.path.getsize(os.path.join(GOLDEN, "ns2d_step_vjp.npz")) < 300 * 1024
    g = load_golden("ns2d_step_vjp.npz")
    assert all(g[k].dtype.kind in "fc" for k in g.files)


def test_new_names_are_declared():
    import torch_cfd_amd as tc
    from torch_cfd_amd import autograd as ad
    from torch_cfd_amd.equations import _HipPlan

    assert len(tc._lib.ADJOINT_SIGNATURES["tcfd_ns2d_step_vjp"][1]) == 18
    assert len(tc._lib.ADJOINT_SIGNATURES["tcfd_ns2d_step_vjp_workspace_bytes"][1]) == 3
    assert not set(tc._lib.ADJOINT_SIGNATURES) & set(tc._lib.SIGNATURES)
    lib = tc._lib.load()
    assert lib.tcfd_ns2d_step_vjp.argtypes == tc._lib.ADJOINT_SIGNATURES["tcfd_ns2d_step_vjp"][1]
    assert hasattr(lib, "tcfd_ns2d_step_vjp") and hasattr(lib, "tcfd_ns2d_step_vjp_workspace_bytes")
    assert lib.tcfd_version() == 13            # added without a new ABI number
    assert lib.tcfd_ns2d_step_vjp_workspace_bytes(None, 4, 5) == 0
    for name in ("adjoint_step", "tangent_step"):
        assert callable(getattr(tc.NavierStokes2DSpectral, name, None)), name
    for name in ("step_vjp", "step_vjp_workspace"):
        assert callable(getattr(_HipPlan, name, None)), name
    assert issubclass(ad.FusedSteps, torch.autograd.Function)


def test_adjoint_header_is_plain_c_and_mirrored():
    """include/tcfd_ns2d_adjoint.h against _lib.ADJOINT_SIGNATURES and the library's exports (what tests/test_abi.py does for
    tcfd.h): the same names, argument counts and the workspace tail; and the header compiles as C99 on its own."""
    import ctypes
    import re
    import shutil
    import subprocess

    import torch_cfd_amd as tc
    from conftest import ROOT

    path = os.path.join(ROOT, "include", "tcfd_ns2d_adjoint.h")
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = dict(re.findall(r"\b(tcfd_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert sorted(protos) == sorted(tc._lib.ADJOINT_SIGNATURES)
    lib = tc._lib.load()
    for name, args in protos.items():
        assert hasattr(lib, name), f"{name} declared but not exported"
        assert len(args.split(",")) == len(tc._lib.ADJOINT_SIGNATURES[name][1]), name
    assert re.search(r"void\*\s+workspace,\s*size_t\s+workspace_bytes,\s*void\*\s+stream$", protos["tcfd_ns2d_step_vjp"].strip())
    assert tc._lib.ADJOINT_SIGNATURES["tcfd_ns2d_step_vjp"][1][-3:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc: the C99 compile of include/tcfd_ns2d_adjoint.h was not checked (everything above was)")
    r = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-Werror", path],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_refusals_that_need_no_device():
    """NULL plan and arguments, steps and nstages out of range: TCFD_EINVAL with a message, before anything touches a device."""
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    one = tc._lib.darray([0.0] * 5)
    rc = lib.tcfd_ns2d_step_vjp(None, None, None, None, None, None, 1, 5, None, one, one, one, None, None, 1, None, 0, None)
    assert rc == -1 and b"null" in lib.tcfd_last_error()


def _cpu_op(n=16, solver=True):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    return tc.NavierStokes2DSpectral(1e-3, grid, solver=tc.RK4CrankNicolsonStepper() if solver else None)


def test_argument_checks_come_before_any_device_call():
    """Mismatched shapes / dtypes and bad counts are a ValueError whatever the device; well-formed CPU tensors reach the plan and
    raise TcfdError (no CPU fallback); without a solver a TypeError."""
    import torch_cfd_amd as tc

    op = _cpu_op()
    w = torch.randn(2, 16, 9, dtype=torch.complex64)
    with pytest.raises(ValueError):
        op.adjoint_step(w, w[:1], 1e-3)
    with pytest.raises(ValueError):
        op.adjoint_step(w, w.to(torch.complex128), 1e-3)
    with pytest.raises(ValueError):
        op.adjoint_step(w[..., :8], w[..., :8], 1e-3)
    with pytest.raises(ValueError):
        op.adjoint_step(w.real, w.real, 1e-3)
    with pytest.raises(ValueError):
        op.adjoint_step(w, w, 1e-3, g_dwdt=w[:1])
    with pytest.raises(ValueError):
        op.adjoint_step(w, w, 1e-3, steps=0)
    with pytest.raises(ValueError):
        op.adjoint_step(w, w, 1e-3, checkpoint_every=0)
    with pytest.raises(NotImplementedError, match="requires grad"):
        op.adjoint_step(w, w.clone().requires_grad_(True), 1e-3)
    with pytest.raises(tc._lib.TcfdError):
        op.adjoint_step(w, w, 1e-3)
    with pytest.raises(TypeError):
        _cpu_op(solver=False).adjoint_step(w, w, 1e-3)
