"""Host-side checks of the tangent-linear spectral step (no GPU): the forward-mode references the GPU tests use -- the CPU
oracle under torch.autograd.forward_ad and the plain-torch restatement tests/ns2d_ops.py -- against the goldens made from the
reference (tests/golden/ns2d_jvp.npz), the new names of the ABI and of the operator, and the argument checks that run before
any device call."""
import math
import os
import sys

import pytest
import torch
import torch.autograd.forward_ad as fwAD

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ns2d_ops  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402

L = 2 * math.pi
FORCINGS = ("none", "kolmogorov", "sincos")
IMEX = {"imex1": (1, 1.0, 1.0), "imex1.5": (1.5, 0.5, 0.5), "imex2": (2, 0.5, 0.5)}


def _golden(prefix=""):
    g = load_golden("ns2d_jvp.npz")
    return g, torch.from_numpy(g[prefix + "w0"]), torch.from_numpy(g[prefix + "dw"]), float(g["dt"])


def _tangent(fn, w, dw):
    return ns2d_ops.jvp(fn, w, dw)[1]


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", FORCINGS)
def test_oracle_forward_mode_tangents_match_the_reference(forcing, smooth):
    """oracle/ns2d.py under forward_ad against the reference's own forward-mode tangents: explicit terms, RK4-CN at 1 and 3
    steps (fp64, n = 16, B = 2).  Bound: 1e-12 -- both are the same fp64 torch ops up to association."""
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float64)
    g, w0, dw, dt = _golden()
    t = ns2d_ops.tables(16, forcing, smooth)
    key = f"{forcing}_s{int(smooth)}_"
    assert rel_l2(_tangent(lambda w: O.explicit_terms(w, t.oracle), w0, dw), g[key + "F"]) <= 1e-12
    for steps in (1, 3):
        got = _tangent(lambda w: O.advance(w, dt, t.oracle, steps=steps)[0], w0, dw)
        assert rel_l2(got, g[key + f"rk{steps}"]) <= 1e-12


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", FORCINGS)
def test_torch_op_restatement_matches_the_oracle_and_the_reference(forcing, smooth):
    """tests/ns2d_ops.py: its explicit terms and RK4-CN steps equal the oracle's (values and tangents), and its stage loop on the
    package's IMEX schedules reproduces the reference's forward-mode tangents of IMEXStepper orders 1, 1.5 and 2 (2 steps)."""
    import torch_cfd_amd as tc
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float64)
    g, w0, dw, dt = _golden()
    t = ns2d_ops.tables(16, forcing, smooth)
    key = f"{forcing}_s{int(smooth)}_"
    f, df = ns2d_ops.jvp(lambda w: ns2d_ops.explicit_terms(w, t), w0, dw)
    assert rel_l2(f, O.explicit_terms(w0, t.oracle)) <= 1e-13
    assert rel_l2(df, g[key + "F"]) <= 1e-12
    rk = ns2d_ops.schedule(tc.RK4CrankNicolsonStepper(), dt)
    w3, dw3 = ns2d_ops.jvp(lambda w: ns2d_ops.advance(w, t, rk, 3), w0, dw)
    assert rel_l2(w3, O.advance(w0, dt, t.oracle, steps=3)[0]) <= 1e-13
    assert rel_l2(dw3, g[key + "rk3"]) <= 1e-12
    for name, (order, alpha, beta) in IMEX.items():
        sched = ns2d_ops.schedule(tc.IMEXStepper(order=order, alpha=alpha, beta=beta), dt)
        got = _tangent(lambda w: ns2d_ops.advance(w, t, sched, 2), w0, dw)
        assert rel_l2(got, g[key + name]) <= 1e-12, name


def test_oracle_forward_mode_tangent_in_single_precision():
    """The complex64 golden (a float32 run of the reference).  Bound 2e-5, the project's fp32 bound: the oracle and the
    reference associate their float32 products differently, each rounding at 6e-8 over some hundred operations per step."""
    from oracle import ns2d as O

    torch.set_default_dtype(torch.float32)
    g, w0, dw, dt = _golden("f32_")
    assert w0.dtype == torch.complex64
    t = ns2d_ops.tables(16, "kolmogorov", True, real=torch.float32)
    assert rel_l2(_tangent(lambda w: O.explicit_terms(w, t.oracle), w0, dw), g["f32_kolmogorov_s1_F"]) <= 2e-5
    got = _tangent(lambda w: O.advance(w, dt, t.oracle, steps=3)[0], w0, dw)
    assert got.dtype == torch.complex64 and rel_l2(got, g["f32_kolmogorov_s1_rk3"]) <= 2e-5


def test_golden_is_small_and_numeric():
    from conftest import GOLDEN

    assert os.path.getsize(os.path.join(GOLDEN, "ns2d_jvp.npz")) < 300 * 1024
    g = load_golden("ns2d_jvp.npz")
    assert all(g[k].dtype.kind in "fc" for k in g.files)


def test_new_names_are_declared():
    import torch_cfd_amd as tc

    for name in ("tcfd_ns2d_explicit_terms_jvp", "tcfd_ns2d_step_jvp", "tcfd_ns2d_jvp_workspace_bytes"):
        assert name in tc._lib.SIGNATURES, name
    assert len(tc._lib.SIGNATURES["tcfd_ns2d_step_jvp"][1]) == 17
    assert len(tc._lib.SIGNATURES["tcfd_ns2d_explicit_terms_jvp"][1]) == 9
    for name in ("explicit_terms_jvp", "tangent_step"):
        assert callable(getattr(tc.NavierStokes2DSpectral, name, None)), name


def _cpu_op(n=16):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    return tc.NavierStokes2DSpectral(1e-3, grid, solver=tc.RK4CrankNicolsonStepper())


def test_argument_checks_come_before_any_device_call():
    """Mismatched shapes / dtypes are a ValueError whatever the device; well-formed CPU tensors reach the plan and raise
    TcfdError (no CPU fallback) -- as explicit calls and as dual numbers."""
    import torch_cfd_amd as tc

    op = _cpu_op()
    w = torch.randn(2, 16, 9, dtype=torch.complex64)
    with pytest.raises(ValueError):
        op.tangent_step(w, w[:1], 1e-3)
    with pytest.raises(ValueError):
        op.explicit_terms_jvp(w, w[..., :8])
    with pytest.raises(ValueError):
        op.tangent_step(w, w.to(torch.complex128), 1e-3)
    with pytest.raises(ValueError):
        op.explicit_terms_jvp(w.real, w.real)
    with pytest.raises(ValueError):
        op.tangent_step(w[..., :8], w[..., :8], 1e-3)
    with pytest.raises(tc._lib.TcfdError):
        op.tangent_step(w, w, 1e-3)
    with pytest.raises(tc._lib.TcfdError):
        op.explicit_terms_jvp(w, w)
    with fwAD.dual_level():
        dual = fwAD.make_dual(w, w.clone())
        with pytest.raises(tc._lib.TcfdError):
            op(dual, 1e-3)
        with pytest.raises(tc._lib.TcfdError):
            op.explicit_terms(dual)


def test_tangent_step_needs_a_solver():
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(16, 16), domain=((0, L), (0, L)))
    op = tc.NavierStokes2DSpectral(1e-3, grid)
    w = torch.randn(16, 9, dtype=torch.complex64)
    with pytest.raises(TypeError):
        op.tangent_step(w, w, 1e-3)
