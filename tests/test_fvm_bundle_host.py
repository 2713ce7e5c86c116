"""CPU-only tests of the finite-volume tangent bundle: the QR step ``orthonormalize_velocity_tangents``, the checks of
``tangent_bundle_step`` / ``explicit_terms_jvp_bundle`` that run before any device call, and the new name of the C ABI
(include/tcfd_fvm_bundle.h against _lib.FVM_BUNDLE_SIGNATURES and the library's exports).

Bounds of the QR: a Householder factorisation is orthogonal to a small multiple of K eps whatever the conditioning of its input,
and backward stable; 100 K eps is asserted for both, on matrices of condition number up to 1e10."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2 * math.pi


# ----------------------------------------------------------------------------- 9. the QR step
def _gram(p, q):
    """<p[j], q[k]> in the cell-sum inner product: (K, K) or (B, K, K)."""
    if p[0].dim() == 3:
        return sum(torch.einsum("jxy,kxy->jk", a, b) for a, b in zip(p, q))
    return sum(torch.einsum("jbxy,kbxy->bjk", a, b) for a, b in zip(p, q))


def _times(q, R):
    if q[0].dim() == 3:
        return tuple(torch.einsum("jxy,jk->kxy", c, R) for c in q)
    return tuple(torch.einsum("jbxy,bjk->kbxy", c, R) for c in q)


def _check_qr(dV, tol):
    import torch_cfd_amd as tc

    (qx, qy), R = tc.orthonormalize_velocity_tangents(dV)
    K = dV[0].shape[0]
    assert qx.shape == dV[0].shape and qy.shape == dV[1].shape and qx.dtype == dV[0].dtype
    assert R.shape == ((K, K) if dV[0].dim() == 3 else (dV[0].shape[1], K, K))
    eye = torch.eye(K, dtype=R.dtype)
    assert float((_gram((qx, qy), (qx, qy)) - eye).abs().max()) <= tol
    back = _times((qx, qy), R)
    scale = max(float(c.abs().max()) for c in dV)
    assert max(float((b - c).abs().max()) for b, c in zip(back, dV)) <= tol * scale
    assert float(torch.tril(R, -1).abs().max()) == 0.0
    assert bool((torch.diagonal(R, dim1=-2, dim2=-1) > 0).all())
    return (qx, qy), R


@pytest.mark.parametrize("shape", [(4, 12, 12), (4, 3, 12, 12), (1, 8, 8), (5, 1, 6, 6)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_orthonormalize_velocity_tangents(shape, dtype):
    gen = torch.Generator().manual_seed(sum(shape))
    dV = tuple(torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype) for _ in range(2))
    _check_qr(dV, 100 * shape[0] * torch.finfo(dtype).eps)


def test_orthonormalize_gives_a_positive_diagonal_for_a_flipped_member():
    gen = torch.Generator().manual_seed(3)
    dV = tuple(torch.randn(3, 8, 8, generator=gen, dtype=torch.float64) for _ in range(2))
    (qx, qy), R = _check_qr(dV, 1e-13)
    flipped = tuple(torch.stack([-c[0], c[1], -c[2]]) for c in dV)
    (fx, fy), Rf = _check_qr(flipped, 1e-13)
    assert torch.allclose(fx[0], -qx[0], atol=1e-13) and torch.allclose(Rf.diagonal(), R.diagonal(), atol=1e-12)


@pytest.mark.parametrize("shape", [(4, 12, 12), (4, 2, 12, 12)])
def test_nearly_parallel_tangents_keep_orthogonality(shape):
    """Every member is the leading vector plus 1e-10 of something else: a condition number of 1e10, the state of a Lyapunov
    bundle after a long interval.  Gram-Schmidt would lose ten digits of orthogonality here."""
    gen = torch.Generator().manual_seed(11)
    lead = tuple(torch.randn(*shape[1:], generator=gen, dtype=torch.float64) for _ in range(2))
    dV = tuple(torch.stack([l + (1e-10 * torch.randn(*shape[1:], generator=gen, dtype=torch.float64) if k else 0)
                            for k in range(shape[0])]) for l in lead)
    M = torch.stack(dV, dim=-3).reshape(shape[0], -1, 2 * shape[-1] ** 2)
    cond = torch.linalg.cond(M[:, 0].T)
    assert float(cond) > 1e9
    _check_qr(dV, 100 * shape[0] * torch.finfo(torch.float64).eps)


def test_orthonormalize_refuses_bad_shapes():
    import torch_cfd_amd as tc

    z = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", torch.float64))
    for bad in ((z(8, 8), z(8, 8)),                      # no member index
                (z(2, 2, 2, 8, 8), z(2, 2, 2, 8, 8)),    # too many dimensions
                (z(3, 8, 6), z(3, 8, 6)),                # not square
                (z(3, 8, 8), z(2, 8, 8)),                # components differ
                (z(3, 8, 8), z(3, 8, 8, dtype=torch.float32)),
                (z(3, 8, 8),),                           # not a pair
                (z(0, 8, 8), z(0, 8, 8)),                # K = 0
                (z(9, 2, 2), z(9, 2, 2)),                # more members than dimensions
                (z(3, 8, 8).long(), z(3, 8, 8).long())):
        with pytest.raises(ValueError):
            tc.orthonormalize_velocity_tangents(bad)


# ----------------------------------------------------------------------------- 10. refusals before any device call
def _equation(solver="classic_rk4", requires_grad=False, viscosity=1e-3, drag=0.1):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(32, 32), domain=((0, L), (0, L)))
    s = None if solver is None else tc.RKStepper.from_method(method=solver, requires_grad=requires_grad)
    return tc.NavierStokes2DFVMProjection(viscosity, grid, drag=drag, solver=s)


def _zeros(*shape, dtype=torch.float64, **kw):
    return (torch.zeros(*shape, dtype=dtype, **kw), torch.zeros(*shape, dtype=dtype, **kw))


def test_the_new_names_are_public():
    import torch_cfd_amd as tc

    for name in ("explicit_terms_jvp_bundle", "tangent_bundle_step"):
        assert callable(getattr(tc.NavierStokes2DFVMProjection, name, None)), name
    assert callable(tc.orthonormalize_velocity_tangents) and tc.orthonormalize_velocity_tangents is tc.fvm.orthonormalize_velocity_tangents


def test_tangent_bundle_step_without_a_solver_raises():
    with pytest.raises(ValueError, match="RKStepper"):
        _equation(None).tangent_bundle_step(_zeros(32, 32), _zeros(3, 32, 32), 0.01)


@pytest.mark.parametrize("call", ["explicit_terms_jvp_bundle", "tangent_bundle_step"])
def test_argument_checks_precede_any_device_call(call):
    """On CPU tensors a device call would raise TcfdError (no CPU fallback): every refusal below comes first, and in the order
    shapes and dtypes -> gradients -> ensemble -> tableau."""
    import torch_cfd_amd as tc

    eq = _equation(requires_grad=True)   # a tableau that requires grad: refused last
    fn = getattr(eq, call)
    u = _zeros(32, 32)
    for bad in (_zeros(32, 32),                    # no member index
                _zeros(3, 2, 32, 32),              # the trailing shape is not the state's
                _zeros(3, 32, 16),
                _zeros(0, 32, 32),                 # K = 0
                (torch.zeros(3, 32, 32, dtype=torch.float64),)):
        with pytest.raises(ValueError):
            fn(u, bad, 0.01)
    with pytest.raises(ValueError, match="K = 0"):
        fn(u, _zeros(0, 32, 32), 0.01)
    with pytest.raises(ValueError, match="tangent must have the shape and dtype"):
        fn(u, _zeros(3, 32, 32, dtype=torch.float32), 0.01)
    with pytest.raises(ValueError, match="n = 32"):
        fn(_zeros(16, 16), _zeros(3, 16, 16), 0.01)
    with pytest.raises(ValueError):
        fn(_zeros(2, 32, 32, dtype=torch.float16), _zeros(3, 2, 32, 32, dtype=torch.float16), 0.01)
    for bad_u, bad_dV in ((_zeros(32, 32, requires_grad=True), _zeros(3, 32, 32)), (u, _zeros(3, 32, 32, requires_grad=True))):
        with pytest.raises(NotImplementedError, match="forward mode over reverse mode is not implemented"):
            fn(bad_u, bad_dV, 0.01)
        with pytest.raises(ValueError):   # the shape check still comes first
            fn(bad_u, _zeros(3, 2, 32, 32), 0.01)
    dV = _zeros(3, 32, 32)
    if call == "tangent_bundle_step":
        with pytest.raises(NotImplementedError, match="tableau"):
            fn(u, dV, 0.01)
        with torch.no_grad(), pytest.raises(tc._lib.TcfdError):   # nothing left to refuse: the device check
            fn(u, dV, 0.01)
    else:
        with pytest.raises(tc._lib.TcfdError):
            fn(u, dV, 0.01)
    # an ensemble takes exactly its B members
    ens = _equation(viscosity=[1e-3, 2e-3], drag=[0.1, 0.0])
    for bad_u, bad_dV in ((_zeros(3, 32, 32), _zeros(2, 3, 32, 32)), (_zeros(32, 32), _zeros(2, 32, 32))):
        with pytest.raises(ValueError, match="ensemble of B = 2"):
            getattr(ens, call)(bad_u, bad_dV, 0.01)
    with pytest.raises(tc._lib.TcfdError):
        getattr(ens, call)(_zeros(2, 32, 32), _zeros(4, 2, 32, 32), 0.01)


def test_a_library_without_the_entry_is_told_to_rebuild():
    """The entry came without a new ABI number, so a library built before it loads: the plan says what to do."""
    import torch_cfd_amd as tc
    from torch_cfd_amd import fvm

    class Old:
        """The loaded library without the new symbol."""

        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "tcfd_fvm_plan_set_tangent_bundle":
                raise AttributeError(name)
            return getattr(self._lib, name)

    lib = tc._lib.load()
    fvm._require_entry(lib, "tcfd_fvm_plan_set_tangent_bundle", "tangent bundles")   # the library of this tree has it
    old = Old(lib)
    assert not hasattr(old, "tcfd_fvm_plan_set_tangent_bundle") and hasattr(old, "tcfd_fvm_plan_set_tangent")
    with pytest.raises(tc._lib.TcfdError, match=r"built before tangent bundles \(tcfd_fvm_plan_set_tangent_bundle\).*rebuild"):
        fvm._require_entry(old, "tcfd_fvm_plan_set_tangent_bundle", "tangent bundles")


# ----------------------------------------------------------------------------- 11. the C ABI's new header and symbol
def test_bundle_header_is_mirrored_and_exported():
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    sig = tc._lib.FVM_BUNDLE_SIGNATURES
    assert sorted(sig) == ["tcfd_fvm_plan_set_tangent_bundle"]
    assert not set(sig) & (set(tc._lib.SIGNATURES) | set(tc._lib.ADJOINT_SIGNATURES) | set(tc._lib.BUNDLE_SIGNATURES)
                           | set(tc._lib.COBUNDLE_SIGNATURES))
    raw = open(os.path.join(ROOT, "include", "tcfd_fvm_bundle.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = dict(re.findall(r"\b(tcfd_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert sorted(protos) == sorted(sig)
    for name, args in protos.items():
        assert hasattr(lib, name), f"{name} is declared but not exported"
        assert len(args.split(",")) == len(sig[name][1]), name
        assert getattr(lib, name).argtypes == sig[name][1] and getattr(lib, name).restype is sig[name][0]
    assert "int tcfd_fvm_plan_set_tangent_bundle(tcfd_fvm_plan* plan, int ntangents);" in text
    assert f"#define TCFD_FVM_MAX_TANGENTS {tc._lib.TCFD_FVM_MAX_TANGENTS}" in text
    # no new ABI number, no entry of tcfd.h changed: the existing table still mirrors that header (tests/test_abi.py)
    assert lib.tcfd_version() == tc._lib.ABI_VERSION == 13
    assert "tcfd_fvm_plan_set_tangent_bundle" not in open(os.path.join(ROOT, "include", "tcfd.h")).read()


def test_the_setter_refuses_a_null_plan_without_a_device():
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    assert lib.tcfd_fvm_plan_set_tangent_bundle(None, 2) == -1
    assert b"fvm_plan_set_tangent_bundle: null plan" in lib.tcfd_last_error()


def test_bundle_header_is_plain_c():
    """The header compiles as C99 on its own (it includes tcfd.h itself)."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    hdr = os.path.join(ROOT, "include", "tcfd_fvm_bundle.h")
    r = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-Werror", hdr],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
