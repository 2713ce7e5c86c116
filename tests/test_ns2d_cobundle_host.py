"""Host-side checks of the cotangent bundle (K cotangents per trajectory in one adjoint call; no GPU): the names of the ABI
(include/tcfd_ns2d_adjoint_bundle.h against _lib.COBUNDLE_SIGNATURES and the library's exports), what the size function and the
entry points refuse before any device call, the argument checks of ``adjoint_bundle_step``, and the reference the GPU tests use:
K cotangents reversed through the CPU stepper by torch autograd, tied to the golden gradients made from the reference."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ns2d_cobundle_ops as CO  # noqa: E402
import ns2d_ops  # noqa: E402
import ns2d_step_vjp_ops as V  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402

L = 2 * math.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcfd_ns2d_explicit_terms_vjp_bundle", "tcfd_ns2d_step_vjp_bundle", "tcfd_ns2d_step_vjp_bundle_workspace_bytes"]


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


def _cpu_op(n=16, nu=1e-3, solver=True):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    return tc.NavierStokes2DSpectral(nu, grid, solver=tc.RK4CrankNicolsonStepper() if solver else None)


def test_new_names_are_declared():
    import torch_cfd_amd as tc
    from torch_cfd_amd.equations import _HipPlan

    sig = tc._lib.COBUNDLE_SIGNATURES
    assert sorted(sig) == NAMES
    assert len(sig["tcfd_ns2d_step_vjp_bundle"][1]) == 19 and len(sig["tcfd_ns2d_explicit_terms_vjp_bundle"][1]) == 9
    assert len(sig["tcfd_ns2d_step_vjp_bundle_workspace_bytes"][1]) == 4
    assert not set(sig) & (set(tc._lib.SIGNATURES) | set(tc._lib.ADJOINT_SIGNATURES) | set(tc._lib.BUNDLE_SIGNATURES))
    assert callable(getattr(tc.NavierStokes2DSpectral, "adjoint_bundle_step", None))
    for name in ("step_vjp_bundle", "explicit_terms_vjp_bundle"):
        assert callable(getattr(_HipPlan, name, None)), name


def test_header_is_mirrored_and_exported():
    """include/tcfd_ns2d_adjoint_bundle.h against _lib.COBUNDLE_SIGNATURES (names, argument counts, the workspace tail) and the
    library's exports; the entries came without a new ABI number."""
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcfd_ns2d_adjoint_bundle.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(tcfd_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert sorted(protos) == NAMES == sorted(tc._lib.COBUNDLE_SIGNATURES)
    for name, args in protos.items():
        assert hasattr(lib, name), f"{name} is declared but not exported"
        assert len(args.split(",")) == len(tc._lib.COBUNDLE_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == tc._lib.COBUNDLE_SIGNATURES[name][1]
        assert getattr(lib, name).restype is tc._lib.COBUNDLE_SIGNATURES[name][0]
    tail = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    for name in NAMES[:2]:
        assert tc._lib.COBUNDLE_SIGNATURES[name][1][-3:] == tail
    assert lib.tcfd_version() == tc._lib.ABI_VERSION == 13


def test_size_function_and_entry_points_refuse_bad_arguments():
    """Through the loaded library, without a device: without a plan the size function answers 0 whatever the counts (an empty
    batch, a cotangent count outside 1..65535, a stage count outside 1..32 included), and the calls answer a NULL plan with
    TCFD_EINVAL and a message before any device call.  (The same counts with a real plan, and the growth in K and in the batch,
    need a device: tests/test_ns2d_cobundle_gpu.py::test_workspace_grows_with_cotangents_and_batch.)"""
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    size = lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # stands for the arrays only, never for a plan
    for batch, k, nst in ((4, 3, 4), (0, 3, 4), (-1, 3, 4), (4, 0, 4), (4, 65536, 4), (4, -2, 4), (4, 3, 0), (4, 3, 33)):
        assert size(None, batch, k, nst) == 0
    one = tc._lib.darray([0.0] * 4)
    rc = lib.tcfd_ns2d_step_vjp_bundle(None, p, p, p, p, p, 1, 2, 4, None, one, one, one, None, None, 1, p, 64, None)
    assert rc == -1 and b"step_vjp_bundle" in lib.tcfd_last_error() and b"null" in lib.tcfd_last_error()
    rc = lib.tcfd_ns2d_explicit_terms_vjp_bundle(None, p, p, p, 1, 2, p, 64, None)
    assert rc == -1 and b"explicit_terms_vjp_bundle" in lib.tcfd_last_error()


def test_argument_checks_come_before_any_device_call():
    """Shapes, dtypes and counts are a ValueError whatever the device; a cotangent that requires grad is refused; a well-formed CPU
    bundle reaches the plan and raises TcfdError (no CPU fallback); an ensemble operator is refused first, naming the limit;
    without a solver a TypeError."""
    import torch_cfd_amd as tc

    op = _cpu_op()
    w = torch.randn(2, 16, 9, dtype=torch.complex64)
    G = torch.randn(3, 2, 16, 9, dtype=torch.complex64)
    call = lambda a, b, **kw: op.adjoint_bundle_step(a, b, 1e-3, **kw)
    for bad in (w, G[:, :1], G[..., :8], G.to(torch.complex128), G[:0], G.unsqueeze(0), G.real, None):
        with pytest.raises(ValueError):
            call(w, bad)
    with pytest.raises(ValueError):
        call(w.real, torch.randn(3, 2, 16, 9))                       # not a half spectrum
    with pytest.raises(ValueError):
        call(w[..., :8], G[..., :8])                                 # not the operator's grid
    for kw in ({"steps": 0}, {"checkpoint_every": 0}, {"g_dwdt": G[:2]}, {"g_dwdt": w}, {"g_dwdt": G.to(torch.complex128)}):
        with pytest.raises(ValueError):
            call(w, G, **kw)
    with pytest.raises(NotImplementedError, match="requires grad"):
        call(w.clone().requires_grad_(True), G)
    with pytest.raises(NotImplementedError, match="requires grad"):
        call(w, G.clone().requires_grad_(True))
    with pytest.raises(tc._lib.TcfdError):
        call(w, G)
    with pytest.raises(tc._lib.TcfdError):
        call(w[0], G[:, 0])                                          # (n, m) state, (K, n, m) bundle
    torch.set_default_dtype(torch.float64)
    ens = _cpu_op(nu=[1e-3, 2e-3])
    w64, G64 = w.to(torch.complex128), G.to(torch.complex128)
    with pytest.raises(NotImplementedError, match="per-sample parameters"):
        ens.adjoint_bundle_step(w64, G64, 1e-3)
    with pytest.raises(NotImplementedError, match="per-sample parameters"):
        ens.adjoint_bundle_step(w64, G64[..., :8], 1e-3)             # the ensemble is refused before the shapes are looked at
    with pytest.raises(TypeError):
        _cpu_op(solver=False).adjoint_bundle_step(w, G, 1e-3)


@pytest.mark.parametrize("forcing,smooth", [("kolmogorov", True), ("none", False)])
def test_reference_cotangents_are_the_golden_gradients(forcing, smooth):
    """The reference of the GPU tests (ns2d_cobundle_ops.oracle_cobundle: ONE forward evaluation of the CPU stepper, reversed by
    torch autograd once per cotangent, fp64): with the golden's cotangent as member 1 of a bundle of three, member 1 is the
    gradient the reference itself produced (tests/golden/ns2d_step_vjp.npz, n = 16) to 1e-9 for every golden run, the other
    members are their own single evaluations, and a zero member gives zeros."""
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float64)
    g = load_golden("ns2d_step_vjp.npz")
    w0, cot, dt = torch.from_numpy(g["w0"]), torch.from_numpy(g["cot"]), float(g["dt"])
    G = torch.stack([0.5 * cot.flip(0), cot, torch.zeros_like(cot)])
    t = ns2d_ops.tables(16, forcing, smooth)
    key = f"{forcing}_s{int(smooth)}_"
    for what, (solver, steps) in V.GOLDEN_RUNS.items():
        sched = ns2d_ops.schedule(V.make_solver(solver), dt)
        fns = [lambda w: ns2d_ops.advance(w, t, sched, steps)]
        if solver == "rk4":
            fns.append(lambda w: O.advance(w, dt, t.oracle, steps=steps)[0])
        for fn in fns:
            out, Wbar = CO.oracle_cobundle(fn, w0, G)
            assert Wbar.shape == G.shape and out.shape == w0.shape
            assert rel_l2(Wbar[1], g[key + what]) <= 1e-9, what
            single = CO.oracle_cobundle(fn, w0, G[:1])[1][0]
            assert rel_l2(Wbar[0], single) <= 1e-14 and not Wbar[2].abs().max() > 0, what
