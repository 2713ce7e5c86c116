"""Host-side checks of the tangent bundle (K tangents per state in one call; no GPU): the argument checks of the two new
operator methods that run before any device call, the names of the ABI (include/tcfd_ns2d_bundle.h against
_lib.BUNDLE_SIGNATURES and the library's exports), what the size function refuses, the QR of a bundle in the real-field inner
product (orthonormalize_tangents), and the reference the GPU tests use: K tangents of oracle/ns2d.py under forward_ad, stacked,
are its K single-tangent evaluations."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ns2d_bundle_ops as BO  # noqa: E402
import ns2d_ops  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402

L = 2 * math.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


def _cpu_op(n=16, nu=1e-3):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    return tc.NavierStokes2DSpectral(nu, grid, solver=tc.RK4CrankNicolsonStepper())


def test_new_names_are_declared():
    import torch_cfd_amd as tc

    sig = tc._lib.BUNDLE_SIGNATURES
    assert sorted(sig) == ["tcfd_ns2d_bundle_workspace_bytes", "tcfd_ns2d_explicit_terms_jvp_bundle", "tcfd_ns2d_step_jvp_bundle"]
    assert len(sig["tcfd_ns2d_step_jvp_bundle"][1]) == 18 and len(sig["tcfd_ns2d_explicit_terms_jvp_bundle"][1]) == 10
    assert len(sig["tcfd_ns2d_bundle_workspace_bytes"][1]) == 3
    assert not set(sig) & (set(tc._lib.SIGNATURES) | set(tc._lib.ADJOINT_SIGNATURES))
    for name in ("explicit_terms_jvp_bundle", "tangent_bundle_step"):
        assert callable(getattr(tc.NavierStokes2DSpectral, name, None)), name
    assert callable(tc.orthonormalize_tangents)


def test_bundle_header_is_mirrored_and_exported():
    """include/tcfd_ns2d_bundle.h against _lib.BUNDLE_SIGNATURES (names, argument counts, the workspace tail) and the library's
    exports; the entries came without a new ABI number."""
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcfd_ns2d_bundle.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(tcfd_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))
    assert sorted(protos) == sorted(tc._lib.BUNDLE_SIGNATURES)
    for name, args in protos.items():
        assert hasattr(lib, name), f"{name} is declared but not exported"
        assert len(args.split(",")) == len(tc._lib.BUNDLE_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == tc._lib.BUNDLE_SIGNATURES[name][1]
    tail = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    for name in ("tcfd_ns2d_explicit_terms_jvp_bundle", "tcfd_ns2d_step_jvp_bundle"):
        assert tc._lib.BUNDLE_SIGNATURES[name][1][-3:] == tail
    assert lib.tcfd_version() == tc._lib.ABI_VERSION == 13


def test_size_function_and_entry_points_refuse_bad_arguments():
    """Through the loaded library, without a device: no plan, an empty batch or a tangent count outside 1..65535 need no scratch,
    and the calls answer a null plan with TCFD_EINVAL and a message.  (Growth in K and in the batch needs a plan, hence a
    device: tests/test_ns2d_bundle_gpu.py::test_workspace_grows_with_tangents_and_batch.)"""
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    assert lib.tcfd_ns2d_bundle_workspace_bytes(None, 4, 3) == 0
    assert lib.tcfd_ns2d_bundle_workspace_bytes(None, 0, 3) == 0 and lib.tcfd_ns2d_bundle_workspace_bytes(None, 4, 0) == 0
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tcfd_ns2d_explicit_terms_jvp_bundle(None, p, p, p, p, 1, 1, p, 64, None) != 0
    assert b"explicit_terms_jvp_bundle" in lib.tcfd_last_error()
    one = tc._lib.darray([1.0])
    assert lib.tcfd_ns2d_step_jvp_bundle(None, p, p, p, p, 1, 1, 1, None, one, one, one, None, None, 1, p, 64, None) != 0
    assert b"step_jvp_bundle" in lib.tcfd_last_error()


def test_argument_checks_come_before_any_device_call():
    """Shapes and dtypes of the bundle are a ValueError whatever the device; a well-formed CPU bundle reaches the plan and raises
    TcfdError (no CPU fallback); an ensemble operator is refused first, naming the limit."""
    import torch_cfd_amd as tc

    op = _cpu_op()
    w = torch.randn(2, 16, 9, dtype=torch.complex64)
    dW = torch.randn(3, 2, 16, 9, dtype=torch.complex64)
    calls = (lambda a, b: op.tangent_bundle_step(a, b, 1e-3), op.explicit_terms_jvp_bundle)
    for call in calls:
        for bad in (w, dW[:, :1], dW[..., :8], dW.to(torch.complex128), dW[:0], dW.unsqueeze(0), dW.real, None):
            with pytest.raises(ValueError):
                call(w, bad)
        with pytest.raises(ValueError):
            call(w.real, torch.randn(3, 2, 16, 9))                       # not a half spectrum
        with pytest.raises(ValueError):
            call(w[..., :8], dW[..., :8])                                # not the operator's grid
        with pytest.raises(tc._lib.TcfdError):
            call(w, dW)
        with pytest.raises(tc._lib.TcfdError):
            call(w[0], dW[:, 0])                                         # (n, m) state, (K, n, m) bundle
    wg = w.clone().requires_grad_(True)
    for call in calls:
        with pytest.raises(NotImplementedError, match="requires grad"):
            call(wg, dW)
        with pytest.raises(NotImplementedError, match="requires grad"):
            call(w, dW.clone().requires_grad_(True))
    torch.set_default_dtype(torch.float64)
    ens = _cpu_op(nu=[1e-3, 2e-3])
    w64, dW64 = w.to(torch.complex128), dW.to(torch.complex128)
    for call in (lambda a, b: ens.tangent_bundle_step(a, b, 1e-3), ens.explicit_terms_jvp_bundle):
        with pytest.raises(NotImplementedError, match="per-sample parameters"):
            call(w64, dW64)
        with pytest.raises(NotImplementedError, match="per-sample parameters"):
            call(w64, dW64[..., :8])                                     # the ensemble is refused before the shapes are looked at
    grid = tc.Grid(shape=(16, 16), domain=((0, L), (0, L)))
    with pytest.raises(TypeError):
        tc.NavierStokes2DSpectral(1e-3, grid).tangent_bundle_step(w, dW, 1e-3)


@pytest.mark.parametrize("n", [8, 16])
def test_orthonormalize_tangents(n):
    """Random half spectra of real fields (K = 3, B = 2, fp64): irfft2(Q) is orthonormal in physical space, Q R reproduces the
    bundle, R is upper triangular with a positive diagonal -- 1e-12 each; and the unbatched form returns the same numbers."""
    import torch_cfd_amd as tc

    K, B = 3, 2
    gen = torch.Generator().manual_seed(n)
    dW = torch.fft.rfft2(torch.randn(K, B, n, n, generator=gen, dtype=torch.float64))
    Q, R = tc.orthonormalize_tangents(dW, n)
    assert Q.shape == dW.shape and Q.dtype == dW.dtype and R.shape == (B, K, K) and R.dtype == torch.float64
    q = torch.fft.irfft2(Q, s=(n, n))
    gram = torch.einsum("jbxy,kbxy->bjk", q, q)
    assert (gram - torch.eye(K, dtype=torch.float64)).abs().max() <= 1e-12
    back = torch.einsum("jbxy,bjk->kbxy", Q, R.to(Q.dtype))
    assert rel_l2(back, dW) <= 1e-12
    assert (torch.tril(R, -1) == 0).all() and (torch.diagonal(R, dim1=-2, dim2=-1) > 0).all()
    # the weights are what makes it the real-field product: the plain complex dot product of the half spectra is NOT orthonormal
    plain = torch.einsum("jbxy,kbxy->bjk", Q.conj(), Q).real / (n * n)
    assert (plain - torch.eye(K, dtype=torch.float64)).abs().max() > 1e-3
    # log R[k, k] is what Benettin's method sums: the norm of the first tangent, then the distances to the spans before
    x = torch.fft.irfft2(dW, s=(n, n))
    assert torch.allclose(R[:, 0, 0], x[0].flatten(1).norm(dim=1), rtol=1e-13)
    Q1, R1 = tc.orthonormalize_tangents(dW[:, 1], n)
    assert Q1.shape == (K, n, n // 2 + 1) and R1.shape == (K, K)
    assert rel_l2(Q1, Q[:, 1]) <= 1e-12 and rel_l2(R1, R[1]) <= 1e-12
    for bad in (dW.real, dW[..., :-1], dW[0, 0]):
        with pytest.raises(ValueError):
            tc.orthonormalize_tangents(bad, n)
    with pytest.raises(ValueError):
        tc.orthonormalize_tangents(dW, n + 2)


def test_orthonormalize_tangents_odd_grid_and_nearly_parallel_tangents():
    """n = 9 has no Nyquist column (every column but ky = 0 counts twice); tangents 1e-9 apart stay orthonormal to 1e-12."""
    import torch_cfd_amd as tc

    gen = torch.Generator().manual_seed(9)
    x = torch.randn(3, 1, 9, 9, generator=gen, dtype=torch.float64)
    Q, R = tc.orthonormalize_tangents(torch.fft.rfft2(x), 9)
    q = torch.fft.irfft2(Q, s=(9, 9))
    assert (torch.einsum("jbxy,kbxy->bjk", q, q) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-12
    x = torch.randn(3, 1, 16, 16, generator=gen, dtype=torch.float64)
    x[1] = x[0] + 1e-9 * x[1]
    Q, R = tc.orthonormalize_tangents(torch.fft.rfft2(x), 16)
    q = torch.fft.irfft2(Q, s=(16, 16))
    assert (torch.einsum("jbxy,kbxy->bjk", q, q) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-12
    assert 0 < R[0, 1, 1] < 1e-7
    # entries of the ky = 0 and Nyquist columns that no real field produces (the solver's states carry some: its 2/3-rule mask
    # keeps kx = -n/3 without the mirror image) are invisible to irfft2: they stay out of the inner product and ride along
    dW = torch.fft.rfft2(torch.randn(3, 2, 16, 16, generator=gen, dtype=torch.float64))
    dW[..., 0] += 0.05 * torch.view_as_complex(torch.randn(3, 2, 16, 2, generator=gen, dtype=torch.float64))
    dW[..., -1] += 0.05 * torch.view_as_complex(torch.randn(3, 2, 16, 2, generator=gen, dtype=torch.float64))
    Q, R = tc.orthonormalize_tangents(dW, 16)
    q = torch.fft.irfft2(Q, s=(16, 16))
    assert (torch.einsum("jbxy,kbxy->bjk", q, q) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-12
    assert rel_l2(torch.einsum("jbxy,bjk->kbxy", Q, R.to(Q.dtype)), dW) <= 1e-12


@pytest.mark.parametrize("forcing,smooth", [("kolmogorov", True), ("none", False)])
def test_stacked_oracle_tangents_are_the_single_tangent_evaluations(forcing, smooth):
    """The reference of the GPU tests (ns2d_bundle_ops.oracle_bundle: ONE forward_ad evaluation of oracle/ns2d.py with the state
    repeated K times along the batch): its stacked tangents are the K single-tangent evaluations and share their primal -- to
    1e-14, the same fp64 operations sample by sample (a batched CPU FFT may order them otherwise) -- and member 0 is the golden
    made from the reference (tests/golden/ns2d_jvp.npz) to 1e-12."""
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float64)
    g = load_golden("ns2d_jvp.npz")
    w0, dw, dt = torch.from_numpy(g["w0"]), torch.from_numpy(g["dw"]), float(g["dt"])
    dW = torch.stack([dw, 0.5 * dw.flip(0), torch.roll(dw, 3, dims=-2) * (1 + 1j)])
    t = ns2d_ops.tables(16, forcing, smooth)
    key = f"{forcing}_s{int(smooth)}_"
    for fn, name in ((lambda w: O.explicit_terms(w, t.oracle), "F"), (lambda w: O.advance(w, dt, t.oracle, steps=3)[0], "rk3")):
        primal, tangents = BO.oracle_bundle(fn, w0, dW)
        assert tangents.shape == dW.shape
        for k in range(dW.shape[0]):
            p1, t1 = ns2d_ops.jvp(fn, w0, dW[k])
            assert rel_l2(tangents[k], t1) <= 1e-14 and rel_l2(primal, p1) <= 1e-14, k
        assert rel_l2(tangents[0], g[key + name]) <= 1e-12
