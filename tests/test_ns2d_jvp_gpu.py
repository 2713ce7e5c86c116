"""The tangent-linear spectral step on the device (tcfd_ns2d_explicit_terms_jvp / tcfd_ns2d_step_jvp, k_rows_jvp).

References: the goldens made from the reference under torch.autograd.forward_ad (tests/golden/ns2d_jvp.npz, n = 16) and, for the
other sizes, the CPU oracle (oracle/ns2d.py) under forward_ad in fp64 (tied to the goldens by tests/test_ns2d_jvp_host.py).  Bounds (rel-L2 over the reference tangent): fp64 explicit-terms tangent 1e-10, stepped
tangents 1e-9 -- the project's bounds for the VJP of the same quantities; fp32 2e-5 against the fp64 tangent; primal against the
plain fused step 1e-12 / 2e-5.  The adjoint identity against the fused reverse-mode path: 1e-12 / 1e-5 relative to
|J dw| |g|.  Linearity, batch independence and reproducibility are compared bitwise.
"""
import functools
import math

import pytest
import torch
import torch.autograd.forward_ad as fwAD

import ns2d_ops
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

L = 2 * math.pi
REAL = {"f64": torch.float64, "f32": torch.float32}
CPLX = {"f64": torch.complex128, "f32": torch.complex64}
IMEX = {"imex1": (1, 1.0, 1.0), "imex1.5": (1.5, 0.5, 0.5), "imex2": (2, 0.5, 0.5)}


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def build_op(n, tag, forcing, dev, smooth=True, solver=None):
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])
    forcing = None if forcing == "none" else forcing
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    fn = {None: None, "kolmogorov": lambda: tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False),
          "sincos": lambda: tc.SinCosForcing(grid=grid, scale=0.1, k=1.0, diam=L)}[forcing]
    fn = fn() if fn else None
    solver = tc.RK4CrankNicolsonStepper() if solver is None else solver
    return tc.NavierStokes2DSpectral(1e-3, grid, drag=ns2d_ops.DRAG[forcing], smooth=smooth, forcing_fn=fn, solver=solver).to(dev)


def dt_of(n):
    return 1e-3 if n <= 256 else 2.5e-4


def _smooth_fields(n, count, k0, seed):
    """`count` seeded real fields with a Gaussian spectrum of width k0 and unit-order amplitude, as fp64 half spectra."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64)
    env = torch.exp(-(k[:, None] ** 2 + k[None, : n // 2 + 1] ** 2) / (2.0 * k0 * k0))
    w = torch.fft.irfft2(torch.fft.rfft2(torch.randn(count, n, n, generator=gen, dtype=torch.float64)) * env, s=(n, n))
    return torch.fft.rfft2(5.0 * w / w.std())


@functools.lru_cache(maxsize=None)
def inputs(n, tag, B):
    """(w0, dw) on the CPU in the precision of `tag`: smooth random vorticity fields (rms 5) and the half spectrum of a smooth
    real perturbation; up to three distinct samples, repeated with different amplitudes for larger batches."""
    k0 = min(4.0, n / 6.0)
    w0, p0 = _smooth_fields(n, min(B, 3), k0, 1000 + n), _smooth_fields(n, min(B, 3), 1.5 * k0, 2000 + n)
    reps = (B + w0.shape[0] - 1) // w0.shape[0]
    scale = (1 + 0.1 * torch.arange(B, dtype=torch.float64))[:, None, None]
    w0 = w0.repeat(reps, 1, 1)[:B] * scale
    p0 = p0.repeat(reps, 1, 1)[:B] * scale.flip(0)
    return w0.to(CPLX[tag]).contiguous(), p0.to(CPLX[tag]).contiguous()


@functools.lru_cache(maxsize=None)
def reference(n, tag, B, forcing, steps):
    """fp64 forward-mode tangents of the CPU oracle (oracle/ns2d.py: `explicit_terms`, `advance`) under forward_ad, from the
    (possibly fp32) inputs: explicit terms and `steps` RK4-CN steps, computed once per case.  For the fp32 case at n = 64 also
    the oracle's OWN fp32 error: the same oracle functions on float32 tables against their fp64 result."""
    from oracle import ns2d as O

    w0, dw = inputs(n, tag, B)
    out = {}
    torch.set_default_dtype(torch.float64)
    t = ns2d_ops.tables(n, forcing, True).oracle
    w64, d64 = w0.to(torch.complex128), dw.to(torch.complex128)
    out["F"], out["dF"] = ns2d_ops.jvp(lambda w: O.explicit_terms(w, t), w64, d64)
    out["w"], out["dw"] = ns2d_ops.jvp(lambda w: O.advance(w, dt_of(n), t, steps=steps)[0], w64, d64)
    if tag == "f32" and n == 64:
        torch.set_default_dtype(torch.float32)
        t32 = ns2d_ops.tables(n, forcing, True, real=torch.float32).oracle
        got = ns2d_ops.jvp(lambda w: O.advance(w, dt_of(n), t32, steps=steps)[0], w0, dw)[1]
        out["own_f32_error"] = rel_l2(got, out["dw"])
    torch.set_default_dtype(torch.float32)
    return out


# ----------------------------------------------------------------------------- goldens (n = 16)
@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", ["none", "kolmogorov", "sincos"])
def test_golden_tangents_fp64(forcing, smooth, dev):
    import torch_cfd_amd as tc

    g = load_golden("ns2d_jvp.npz")
    dt = float(g["dt"])
    w0, dw = torch.from_numpy(g["w0"]).to(dev), torch.from_numpy(g["dw"]).to(dev)
    key = f"{forcing}_s{int(smooth)}_"
    op = build_op(16, "f64", forcing, dev, smooth)
    f, df = op.explicit_terms_jvp(w0, dw)
    err = rel_l2(df, g[key + "F"])
    print(f"{key}F {err:.3e}")
    assert err <= 1e-10
    assert rel_l2(f, op.explicit_terms(w0)) <= 1e-12
    for steps in (1, 3):
        w, d = op.tangent_step(w0, dw, dt, steps)
        err = rel_l2(d, g[key + f"rk{steps}"])
        print(f"{key}rk{steps} {err:.3e}")
        assert err <= 1e-9
        assert rel_l2(w, op(w0, dt, steps)[0]) <= 1e-12
    for name, (order, alpha, beta) in IMEX.items():
        op = build_op(16, "f64", forcing, dev, smooth, solver=tc.IMEXStepper(order=order, alpha=alpha, beta=beta))
        w, d = op.tangent_step(w0, dw, dt, 2)
        err = rel_l2(d, g[key + name])
        print(f"{key}{name} {err:.3e}")
        assert err <= 1e-9, name
        assert rel_l2(w, op(w0, dt, 2)[0]) <= 1e-12, name


def test_golden_tangents_fp32(dev):
    """complex64 run against the reference's complex64 tangents (both carry fp32 round-off: 2e-5)."""
    g = load_golden("ns2d_jvp.npz")
    dt = float(g["dt"])
    w0, dw = torch.from_numpy(g["f32_w0"]).to(dev), torch.from_numpy(g["f32_dw"]).to(dev)
    op = build_op(16, "f32", "kolmogorov", dev)
    f, df = op.explicit_terms_jvp(w0, dw)
    assert df.dtype == torch.complex64 and rel_l2(df, g["f32_kolmogorov_s1_F"]) <= 2e-5
    w, d = op.tangent_step(w0, dw, dt, 3)
    assert rel_l2(d, g["f32_kolmogorov_s1_rk3"]) <= 2e-5
    assert rel_l2(w, op(w0, dt, 3)[0]) <= 2e-5


# ----------------------------------------------------------------------------- every size against the CPU forward-mode tangent
ORACLE_CASES = [(8, "f64", 3, "kolmogorov", 3), (64, "f64", 3, "kolmogorov", 3), (64, "f32", 3, "kolmogorov", 3),
                (80, "f64", 2, "sincos", 2), (80, "f32", 2, "sincos", 2), (96, "f64", 3, "none", 2), (96, "f32", 3, "none", 2),
                (256, "f64", 2, "kolmogorov", 1), (256, "f32", 2, "kolmogorov", 1), (512, "f64", 1, "none", 1),
                (512, "f32", 1, "kolmogorov", 1), (1024, "f64", 1, "kolmogorov", 1), (1024, "f32", 1, "none", 1)]


@pytest.mark.parametrize("n,tag,B,forcing,steps", ORACLE_CASES)
def test_tangents_against_cpu_forward_mode(n, tag, B, forcing, steps, dev):
    """Smallest fused plan (8), radix-5 / radix-3 first passes (80, 96), the sizes whose plain step runs cross-lane row / column
    kernels and split column plans next to the Stockham passes of the tangent sweep (512, 1024), ragged B = 3; both precisions.
    Explicit-terms tangent and stepped tangent (with the primal) at every size against the CPU oracle under forward_ad."""
    ref = reference(n, tag, B, forcing, steps)
    w0, dw = (x.to(dev) for x in inputs(n, tag, B))
    op = build_op(n, tag, forcing, dev)
    tol_f, tol_s, tol_p = (1e-10, 1e-9, 1e-12) if tag == "f64" else (2e-5, 2e-5, 2e-5)
    f, df = op.explicit_terms_jvp(w0, dw)
    e_f, e_df = rel_l2(f, ref["F"]), rel_l2(df, ref["dF"])
    w, d = op.tangent_step(w0, dw, dt_of(n), steps)
    e_p = rel_l2(w, op(w0, dt_of(n), steps)[0])
    e_w, e_d = rel_l2(w, ref["w"]), rel_l2(d, ref["dw"])
    print(f"n={n} {tag} B={B} {forcing} steps={steps}: F {e_f:.3e} dF {e_df:.3e} w {e_w:.3e} dw {e_d:.3e} primal-vs-step {e_p:.3e}"
          + (f" oracle's own fp32 error {ref['own_f32_error']:.3e}" if "own_f32_error" in ref else ""))
    assert e_df <= tol_f and e_f <= tol_f
    assert e_d <= tol_s and e_w <= tol_s
    assert e_p <= tol_p


# ----------------------------------------------------------------------------- adjoint identity against the fused VJP
@pytest.mark.parametrize("n,tag,B,forcing", [(16, "f64", 3, "kolmogorov"), (64, "f64", 3, "kolmogorov"), (64, "f32", 3, "kolmogorov"),
                                            (80, "f64", 2, "sincos"), (96, "f32", 2, "none"), (256, "f64", 2, "none"),
                                            (512, "f64", 2, "kolmogorov"), (1024, "f64", 1, "none"), (1024, "f32", 1, "kolmogorov")])
def test_adjoint_identity_against_the_fused_vjp(n, tag, B, forcing, dev):
    """<J dw, g> = <dw, J^T g> in the real inner product, J^T g from the existing reverse-mode kernels
    (tcfd_ns2d_explicit_terms_vjp, tcfd_ns2d_stage_update_vjp), for the explicit terms and for one and two steps."""
    w0, dw = (x.to(dev) for x in inputs(n, tag, B))
    op = build_op(n, tag, forcing, dev)
    gen = torch.Generator().manual_seed(n + B)
    g = torch.randn(B, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64)
    g = torch.view_as_complex(g).to(CPLX[tag]).to(dev)
    tol = 1e-12 if tag == "f64" else 1e-5
    dt = dt_of(n)

    def check(what, jdw, forward):
        w = w0.clone().requires_grad_(True)
        jtg, = torch.autograd.grad(ns2d_ops.real_inner(g, forward(w)), w)
        lhs, rhs = ns2d_ops.real_inner(jdw, g).item(), ns2d_ops.real_inner(dw, jtg).item()
        scale = (torch.linalg.norm(jdw) * torch.linalg.norm(g)).item()
        print(f"n={n} {tag} {what}: <Jdw,g> {lhs:.12e} <dw,JTg> {rhs:.12e} defect/scale {abs(lhs - rhs) / scale:.3e}")
        assert abs(lhs - rhs) <= tol * scale, what

    check("explicit", op.explicit_terms_jvp(w0, dw)[1], op.explicit_terms)
    for steps in (1, 2):
        check(f"steps={steps}", op.tangent_step(w0, dw, dt, steps)[1], lambda w: op(w, dt, steps)[0])


# ----------------------------------------------------------------------------- exact properties, bitwise
@pytest.mark.parametrize("n,tag,B,solver", [(16, "f64", 3, "rk4"), (64, "f32", 3, "rk4"), (64, "f64", 3, "imex2"), (96, "f64", 2, "rk4"),
                                            (256, "f32", 3, "imex1.5")])
def test_linearity_and_reproducibility_bitwise(n, tag, B, solver, dev):
    import torch_cfd_amd as tc

    stepper = None if solver == "rk4" else tc.IMEXStepper(order=IMEX[solver][0], alpha=IMEX[solver][1], beta=IMEX[solver][2])
    op = build_op(n, tag, "kolmogorov", dev, solver=stepper)
    w0, dw = (x.to(dev) for x in inputs(n, tag, B))
    dt = dt_of(n)
    w1, d1 = op.tangent_step(w0, dw, dt, 3)
    # a second run gives the same bits
    w1b, d1b = op.tangent_step(w0, dw, dt, 3)
    assert torch.equal(w1, w1b) and torch.equal(d1, d1b)
    # zero tangent -> zero tangent; the primal does not depend on the tangent
    wz, dz = op.tangent_step(w0, torch.zeros_like(dw), dt, 3)
    assert (dz == 0).all() and torch.equal(wz, w1)
    fz, dfz = op.explicit_terms_jvp(w0, torch.zeros_like(dw))
    assert (dfz == 0).all()
    # exact homogeneity in the tangent (a power of two scales every intermediate exactly)
    w2, d2 = op.tangent_step(w0, 2 * dw, dt, 3)
    assert torch.equal(w2, w1) and torch.equal(d2, 2 * d1)
    f1, df1 = op.explicit_terms_jvp(w0, dw)
    f2, df2 = op.explicit_terms_jvp(w0, 2 * dw)
    assert torch.equal(f1, f2) and torch.equal(f1, fz) and torch.equal(df2, 2 * df1)
    # steps = K equals K one-step calls
    ws, ds = w0, dw
    for _ in range(3):
        ws, ds = op.tangent_step(ws, ds, dt, 1)
    assert torch.equal(ws, w1) and torch.equal(ds, d1)
    # every sample of the batch equals its run alone
    for b in range(B):
        wa, da = op.tangent_step(w0[b:b + 1], dw[b:b + 1], dt, 3)
        assert torch.equal(wa[0], w1[b]) and torch.equal(da[0], d1[b]), b


@pytest.mark.parametrize("n,B", [(1024, 6), (512, 20)])
def test_several_chunks_per_call_equal_the_samples_alone(n, B, dev):
    """fp64 batches the library cuts into several chunks (a chunk of the tangent calls holds half the fields of a chunk of the
    plain step): every sample must carry the bits of its run alone, and a second run the same bits."""
    import ctypes

    op = build_op(n, "f64", "kolmogorov", dev)
    w0, dw = (x.to(dev) for x in inputs(n, "f64", B))
    plan = op._plan(w0)
    per = ctypes.c_long(0)
    plan.lib.tcfd_ns2d_plan_chunking(plan.handle, 2 * B, ctypes.byref(per), None, None)
    assert per.value < 2 * B, "the case is meant to run in several chunks"
    dt = dt_of(n)
    w1, d1 = op.tangent_step(w0, dw, dt, 1)
    f1, df1 = op.explicit_terms_jvp(w0, dw)
    w1b, d1b = op.tangent_step(w0, dw, dt, 1)
    assert torch.equal(w1, w1b) and torch.equal(d1, d1b)
    for b in range(B):
        wa, da = op.tangent_step(w0[b:b + 1], dw[b:b + 1], dt, 1)
        fa, dfa = op.explicit_terms_jvp(w0[b:b + 1], dw[b:b + 1])
        assert torch.equal(wa[0], w1[b]) and torch.equal(da[0], d1[b]), b
        assert torch.equal(fa[0], f1[b]) and torch.equal(dfa[0], df1[b]), b
    assert rel_l2(w1, op(w0, dt, 1)[0]) <= 1e-12


# ----------------------------------------------------------------------------- shapes, dual numbers, errors
def test_input_shapes_and_the_empty_batch(dev):
    op = build_op(64, "f64", "kolmogorov", dev)
    w0, dw = (x.to(dev) for x in inputs(64, "f64", 4))
    w, d = op.tangent_step(w0, dw, 1e-3, 2)
    w1, d1 = op.tangent_step(w0[0], dw[0], 1e-3, 2)
    assert w1.shape == (64, 33) and torch.equal(w1, w[0]) and torch.equal(d1, d[0])
    w4, d4 = op.tangent_step(w0.reshape(2, 2, 64, 33), dw.reshape(2, 2, 64, 33), 1e-3, 2)
    assert w4.shape == (2, 2, 64, 33) and torch.equal(w4.reshape(4, 64, 33), w) and torch.equal(d4.reshape(4, 64, 33), d)
    f4, df4 = op.explicit_terms_jvp(w0.reshape(2, 2, 64, 33), dw.reshape(2, 2, 64, 33))
    assert df4.shape == (2, 2, 64, 33) and torch.equal(df4.reshape(4, 64, 33), op.explicit_terms_jvp(w0, dw)[1])
    we, de = op.tangent_step(w0[:0], dw[:0], 1e-3)
    assert we.shape == (0, 64, 33) and de.shape == (0, 64, 33)
    fe, dfe = op.explicit_terms_jvp(w0[:0], dw[:0])
    assert fe.shape == (0, 64, 33) and dfe.shape == (0, 64, 33)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_dual_inputs_return_the_bits_of_the_explicit_calls(tag, dev):
    import torch_cfd_amd as tc

    op = build_op(64, tag, "kolmogorov", dev)
    w0, dw = (x.to(dev) for x in inputs(64, tag, 3))
    dt, steps = 1e-3, 2
    ref_w, ref_d = op.tangent_step(w0, dw, dt, steps)
    ref_f, ref_df = op.explicit_terms_jvp(w0, dw)
    plain_w, plain_dwdt = op(w0, dt, steps)
    with fwAD.dual_level():
        dual = fwAD.make_dual(w0, dw)
        for call in (op, op.step):
            new, dwdt = call(dual, dt, steps)
            new, dwdt = fwAD.unpack_dual(new), fwAD.unpack_dual(dwdt)
            assert torch.equal(new.primal, ref_w) and torch.equal(new.tangent, ref_d)
            assert torch.equal(dwdt.tangent, (ref_d - dw) / (steps * dt))
            assert torch.equal(dwdt.primal, (ref_w - w0) / (steps * dt))
        f = fwAD.unpack_dual(op.explicit_terms(dual))
        assert torch.equal(f.primal, ref_f) and torch.equal(f.tangent, ref_df)
        # the stepper called directly, as a foreign time loop would
        one = fwAD.unpack_dual(op.solver(dual, dt, op))
        w1, d1 = op.tangent_step(w0, dw, dt, 1)
        assert torch.equal(one.primal, w1) and torch.equal(one.tangent, d1)
        # an input without a tangent takes the plain path, inside a dual level too
        new, dwdt = op(w0, dt, steps)
        assert fwAD.unpack_dual(new).tangent is None and torch.equal(new, plain_w) and torch.equal(dwdt, plain_dwdt)

        # a foreign solver(u, dt, equation) works through explicit_terms on its own
        class Foreign:
            def __call__(self, u, dt, equation):
                return tc.run_stage_schedule(u, equation, op.solver.stage_schedule(op.solver.params, dt))

        foreign = build_op(64, tag, "kolmogorov", dev, solver=Foreign())
        new, _ = foreign(dual, dt, steps)
        new = fwAD.unpack_dual(new)
        tol = 1e-12 if tag == "f64" else 2e-5
        assert new.tangent is not None and rel_l2(new.tangent, ref_d) <= tol and rel_l2(new.primal, ref_w) <= tol
    # residual of a dual state keeps its tangent: d(res) = d(w_t) - F'(w) dw - L dw
    with fwAD.dual_level():
        res = fwAD.unpack_dual(op.residual(fwAD.make_dual(w0, dw), fwAD.make_dual(plain_dwdt, torch.zeros_like(dw))))
        want = -ref_df - op.linear_term * dw
        assert res.tangent is not None and rel_l2(res.tangent, want) <= (1e-12 if tag == "f64" else 2e-5)


def test_unsupported_combinations_raise(dev):
    """Never a silently dropped tangent: NotImplementedError naming the limit."""
    import torch_cfd_amd as tc

    op = build_op(64, "f64", "kolmogorov", dev)
    w0, dw = (x.to(dev) for x in inputs(64, "f64", 2))
    # 1. a dual input that also requires grad in grad mode
    wg = w0.clone().requires_grad_(True)
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="requires grad"):
            op(fwAD.make_dual(wg, dw), 1e-3)
        with pytest.raises(NotImplementedError, match="requires grad"):
            op.explicit_terms(fwAD.make_dual(wg, dw))
        with torch.no_grad():   # without grad mode it is a plain tangent
            new, _ = op(fwAD.make_dual(wg, dw), 1e-3)
            assert fwAD.unpack_dual(new).tangent is not None
    with pytest.raises(NotImplementedError, match="requires grad"):
        op.tangent_step(wg, dw, 1e-3)
    # 2. trainable stepper coefficients together with a tangent
    trainable = build_op(64, "f64", "kolmogorov", dev, solver=tc.RK4CrankNicolsonStepper(requires_grad=True))
    with pytest.raises(NotImplementedError, match="trainable"):
        trainable.tangent_step(w0, dw, 1e-3)
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="trainable"):
            trainable(fwAD.make_dual(w0, dw), 1e-3)
    # 3. a grid outside the fused sizes
    small = build_op(48, "f64", "none", dev)
    w48 = torch.fft.rfft2(torch.randn(2, 48, 48, dtype=torch.float64)).to(dev)
    with pytest.raises(NotImplementedError, match="fused grid sizes"):
        small.tangent_step(w48, w48.clone(), 1e-3)
    with pytest.raises(NotImplementedError, match="fused grid sizes"):
        small.explicit_terms_jvp(w48, w48.clone())
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="fused grid sizes"):
            small(fwAD.make_dual(w48, w48.clone()), 1e-3)
    # the library refuses a short workspace instead of writing past it
    plan = op._plan(w0)
    out, dout = torch.empty_like(w0), torch.empty_like(w0)
    ws = torch.empty(1024, dtype=torch.uint8, device=dev)
    rc = plan.lib.tcfd_ns2d_explicit_terms_jvp(plan.handle, w0.data_ptr(), dw.data_ptr(), out.data_ptr(), dout.data_ptr(), 2,
                                               ws.data_ptr(), ws.numel(), None)
    assert rc != 0
