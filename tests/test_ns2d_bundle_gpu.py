"""K tangents per state in one call on the device (tcfd_ns2d_explicit_terms_jvp_bundle / tcfd_ns2d_step_jvp_bundle,
k_rows_jvp_bundle and the two-pass fall-back): NavierStokes2DSpectral.explicit_terms_jvp_bundle / tangent_bundle_step.

References: the CPU oracle (oracle/ns2d.py) in fp64 under forward_ad, one evaluation per bundle (ns2d_bundle_ops.oracle_bundle,
tied to its single-tangent evaluations and to the goldens by tests/test_ns2d_bundle_host.py); the IMEX schedules through
tests/ns2d_ops.py (tied to the reference's IMEX tangents by tests/test_ns2d_jvp_host.py); the single-tangent calls of the same
build; the adjoint model.  Bounds are the project's: explicit-terms tangents 1e-10 (fp64) / 2e-5 (fp32) relative
L2 against the fp64 oracle, stepped tangents 1e-9 / 2e-5, the state against the plain fused step 1e-12, member k against
tangent_step alone 1e-12 / 2e-5 (whether the bits are equal is printed; DESIGN 23 says where they are), the adjoint
identity 1e-12 / 1e-5 of |J dw_k| |g|.  Independence, homogeneity, chunking and reproducibility are compared bitwise.

Sizes: 8 (smallest plan), 16, 64; 80 (fp64: two-pass fall-back, fp32: 20 elements per lane in the bundle kernel), 96 (12 per
lane), 160 (5 * 2^k), 1024 (workgroup-wide transforms; fp64 with K = 4: one state per chunk, tangent groups of 2), 1536 (fp64:
fall-back by the LDS rule), 512 x 11 (three chunks, the last one short).
"""
import ctypes
import functools
import math
import re

import pytest
import torch

import ns2d_bundle_ops as BO
import ns2d_ops
import test_ns2d_jvp_gpu as J
from conftest import rel_l2

pytestmark = pytest.mark.gpu

L = 2 * math.pi
IMEX = J.IMEX
TCFD_EINVAL, TCFD_EWORKSPACE = -1, -4      # include/tcfd.h


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def on(dev, *xs):
    return tuple(x.to(dev) for x in xs)


# ----------------------------------------------------------------------------- explicit terms against the oracle
EXPLICIT_CASES = [(n, tag, 2, 3) for n in (8, 16, 64, 80, 96) for tag in ("f64", "f32")] + [
    (1024, "f64", 1, 2), (1024, "f32", 1, 2), (1536, "f64", 1, 2)]


@functools.lru_cache(maxsize=None)
def explicit_reference(n, tag, B, K):
    from oracle import ns2d as O

    w0, dW = BO.inputs(n, tag, B, K)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        t = ns2d_ops.tables(n, "kolmogorov", True).oracle
        return BO.oracle_bundle(lambda w: O.explicit_terms(w, t), w0.to(torch.complex128), dW.to(torch.complex128))
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("n,tag,B,K", EXPLICIT_CASES)
def test_explicit_terms_bundle_against_cpu_forward_mode(n, tag, B, K, dev):
    """F and the K tangents of F against the fp64 oracle under forward_ad: 1e-10 (fp64), 2e-5 (fp32); then member k against
    explicit_terms_jvp alone (1e-12 / 2e-5; bits printed), F against the single call's, and K = 1."""
    F_ref, dF_ref = explicit_reference(n, tag, B, K)
    w0, dW = on(dev, *BO.inputs(n, tag, B, K))
    op = J.build_op(n, tag, "kolmogorov", dev)
    tol, tol_m = (1e-10, 1e-12) if tag == "f64" else (2e-5, 2e-5)
    F, dF = op.explicit_terms_jvp_bundle(w0, dW)
    assert F.shape == w0.shape and dF.shape == dW.shape and dF.dtype == w0.dtype
    e_f, e_d = rel_l2(F, F_ref), [rel_l2(dF[k], dF_ref[k]) for k in range(K)]
    print(f"n={n} {tag} B={B} K={K}: F {e_f:.3e} dF " + " ".join(f"{e:.3e}" for e in e_d))
    assert e_f <= tol and max(e_d) <= tol
    for k in range(K):
        f1, df1 = op.explicit_terms_jvp(w0, dW[k])
        e = rel_l2(dF[k], df1)
        print(f"  member {k} against explicit_terms_jvp alone: {e:.3e} bits equal: {torch.equal(dF[k], df1)}; F bits equal: {torch.equal(F, f1)}")
        assert e <= tol_m and rel_l2(F, f1) <= tol_m
        Fk, dFk = op.explicit_terms_jvp_bundle(w0, dW[k:k + 1])          # K = 1
        assert torch.equal(dFk[0], dF[k]) and torch.equal(Fk, F)


# ----------------------------------------------------------------------------- stepped bundle against the oracle
@functools.lru_cache(maxsize=None)
def stepped_reference(n, tag, forcing, smooth):
    """fp64 references from the (possibly fp32) inputs, B = 2, K = 3: RK4-CN at 1 and 3 steps from the oracle's own stepper, the
    IMEX orders (2 steps) from the stage loop of tests/ns2d_ops.py on the package's schedules."""
    import torch_cfd_amd as tc
    from oracle import ns2d as O

    w0, dW = BO.inputs(n, tag, 2, 3)
    w64, d64 = w0.to(torch.complex128), dW.to(torch.complex128)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        t = ns2d_ops.tables(n, forcing, smooth)
        out = {}
        for steps in (1, 3):
            out[f"rk{steps}"] = BO.oracle_bundle(lambda w: O.advance(w, J.dt_of(n), t.oracle, steps=steps)[0], w64, d64)
        for name, (order, alpha, beta) in IMEX.items():
            sched = ns2d_ops.schedule(tc.IMEXStepper(order=order, alpha=alpha, beta=beta), J.dt_of(n))
            out[name] = BO.oracle_bundle(lambda w: ns2d_ops.advance(w, t, sched, 2), w64, d64)
        return out
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", ["kolmogorov", "none"])
@pytest.mark.parametrize("n", [16, 64])
def test_stepped_bundle_against_cpu_forward_mode(n, forcing, smooth, tag, dev):
    """RK4-CN for 1 and 3 steps and IMEX orders 1, 1.5, 2 (2 steps), forcing and `smooth` on and off.  fp64: tangents 1e-9, the
    state against op(w, dt, steps) 1e-12; fp32: tangents 2e-5 against the fp64 tangents."""
    import torch_cfd_amd as tc

    ref = stepped_reference(n, tag, forcing, smooth)
    w0, dW = on(dev, *BO.inputs(n, tag, 2, 3))
    dt = J.dt_of(n)
    cases = [(f"rk{s}", None, s) for s in (1, 3)] + [(name, tc.IMEXStepper(order=o, alpha=a, beta=b), 2) for name, (o, a, b) in IMEX.items()]
    for name, stepper, steps in cases:
        op = J.build_op(n, tag, forcing, dev, smooth, solver=stepper)
        w, d = op.tangent_bundle_step(w0, dW, dt, steps)
        e_d = max(rel_l2(d[k], ref[name][1][k]) for k in range(3))
        e_w, e_p = rel_l2(w, ref[name][0]), rel_l2(w, op(w0, dt, steps)[0])
        print(f"n={n} {tag} {forcing} smooth={smooth} {name}: tangents {e_d:.3e} state {e_w:.3e} state-vs-step {e_p:.3e}")
        if tag == "f64":
            assert e_d <= 1e-9 and e_w <= 1e-9 and e_p <= 1e-12, name
        else:
            assert e_d <= 2e-5 and e_w <= 2e-5 and e_p <= 2e-5, name


# ----------------------------------------------------------------------------- member k against tangent_step alone
MEMBER_CASES = EXPLICIT_CASES + [(160, "f64", 2, 3), (160, "f32", 2, 3), (1024, "f64", 2, 4)]
# (bits: equal only where both calls run the SAME row kernels -- the fp64 5 * 2^k sizes, two passes in either; elsewhere the
# sums have k_rows_jvp's order but the compiler contracts multiply-adds per kernel, and the two differ in the last place: DESIGN 23)
SAME_ROW_KERNELS = {(80, "f64"), (160, "f64")}


@pytest.mark.parametrize("n,tag,B,K", MEMBER_CASES)
def test_member_k_against_tangent_step_alone(n, tag, B, K, dev):
    """Two RK4-CN steps (one at n >= 1024): member k of the bundle against tangent_step(w, dW[k]), 1e-12 / 2e-5 (bit for bit where
    the two run the same row kernels); the state against tangent_step's; K = 1 gives the member's bits again."""
    w0, dW = on(dev, *BO.inputs(n, tag, B, K))
    op = J.build_op(n, tag, "kolmogorov", dev)
    dt, steps = J.dt_of(n), (2 if n < 1024 else 1)
    tol = 1e-12 if tag == "f64" else 2e-5
    w, d = op.tangent_bundle_step(w0, dW, dt, steps)
    for k in range(K):
        w1, d1 = op.tangent_step(w0, dW[k], dt, steps)
        e, eq = rel_l2(d[k], d1), torch.equal(d[k], d1) and torch.equal(w, w1)
        print(f"n={n} {tag} B={B} K={K} member {k}: {e:.3e} against tangent_step alone, bits equal: {eq}")
        assert e <= tol and rel_l2(w, w1) <= tol
        assert eq or (n, tag) not in SAME_ROW_KERNELS
    wk, dk = op.tangent_bundle_step(w0, dW[K - 1:], dt, steps)
    assert torch.equal(dk[0], d[K - 1]) and torch.equal(wk, w)


# ----------------------------------------------------------------------------- adjoint identity, member by member
@pytest.mark.parametrize("n,tag", [(16, "f64"), (16, "f32"), (64, "f64"), (64, "f32"), (1024, "f64"), (1024, "f32")])
def test_adjoint_identity_per_member(n, tag, dev):
    """<J dw_k, g> = <dw_k, J^T g> in the real inner product, J^T g from adjoint_step (the adjoint model), B = 1, K = 3, two
    steps (one at 1024): 1e-12 (fp64) / 1e-5 (fp32) of |J dw_k| |g|."""
    K = 3
    w0, dW = on(dev, *BO.inputs(n, tag, 1, K))
    op = J.build_op(n, tag, "kolmogorov", dev)
    gen = torch.Generator().manual_seed(n)
    g = torch.view_as_complex(torch.randn(1, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64)).to(w0.dtype).to(dev)
    dt, steps = J.dt_of(n), (2 if n < 1024 else 1)
    tol = 1e-12 if tag == "f64" else 1e-5
    _, d = op.tangent_bundle_step(w0, dW, dt, steps)
    _, jtg = op.adjoint_step(w0, g, dt, steps)
    for k in range(K):
        lhs, rhs = ns2d_ops.real_inner(d[k], g).item(), ns2d_ops.real_inner(dW[k], jtg).item()
        scale = (torch.linalg.norm(d[k]) * torch.linalg.norm(g)).item()
        print(f"n={n} {tag} member {k}: <Jdw,g> {lhs:.12e} <dw,JTg> {rhs:.12e} defect/scale {abs(lhs - rhs) / scale:.3e}")
        assert abs(lhs - rhs) <= tol * scale, k


# ----------------------------------------------------------------------------- exact properties, bitwise
@pytest.mark.parametrize("n,tag,solver", [(64, "f64", "rk4"), (64, "f32", "imex2"), (160, "f64", "rk4"), (160, "f32", "rk4")])
def test_bundle_properties_bitwise(n, tag, solver, dev):
    import torch_cfd_amd as tc

    stepper = None if solver == "rk4" else tc.IMEXStepper(order=IMEX[solver][0], alpha=IMEX[solver][1], beta=IMEX[solver][2])
    op = J.build_op(n, tag, "kolmogorov", dev, solver=stepper)
    B, K = 2, 3
    w0, dW = on(dev, *BO.inputs(n, tag, B, K))
    dt = J.dt_of(n)
    w1, d1 = op.tangent_bundle_step(w0, dW, dt, 3)
    f1, df1 = op.explicit_terms_jvp_bundle(w0, dW)
    # a second run gives the same bits
    w1b, d1b = op.tangent_bundle_step(w0, dW, dt, 3)
    assert torch.equal(w1, w1b) and torch.equal(d1, d1b)
    # a zero member stays zero while the others do not; they and the state keep their bits
    dZ = dW.clone()
    dZ[1] = 0
    wz, dz = op.tangent_bundle_step(w0, dZ, dt, 3)
    fz, dfz = op.explicit_terms_jvp_bundle(w0, dZ)
    assert (dz[1] == 0).all() and (dfz[1] == 0).all()
    assert (dz[0] != 0).any() and torch.equal(dz[0], d1[0]) and torch.equal(dz[2], d1[2]) and torch.equal(wz, w1)
    assert torch.equal(dfz[0], df1[0]) and torch.equal(dfz[2], df1[2]) and torch.equal(fz, f1)
    # exact homogeneity (a power of two scales every intermediate exactly), member by member
    d2in = dW.clone()
    d2in[0] *= 2
    w2, d2 = op.tangent_bundle_step(w0, d2in, dt, 3)
    f2, df2 = op.explicit_terms_jvp_bundle(w0, d2in)
    assert torch.equal(w2, w1) and torch.equal(d2[0], 2 * d1[0]) and torch.equal(d2[1], d1[1]) and torch.equal(d2[2], d1[2])
    assert torch.equal(f2, f1) and torch.equal(df2[0], 2 * df1[0]) and torch.equal(df2[1], df1[1])
    # member k does not depend on the other members, nor the state on any of them
    for k in range(K):
        wk, dk = op.tangent_bundle_step(w0, dW[k:k + 1], dt, 3)
        assert torch.equal(dk[0], d1[k]) and torch.equal(wk, w1), k
    wp, dp = op.tangent_bundle_step(w0, dW.flip(0), dt, 3)
    assert torch.equal(wp, w1) and torch.equal(dp.flip(0), d1)
    assert torch.equal(w1, op(w0, dt, 3)[0]) or rel_l2(w1, op(w0, dt, 3)[0]) <= (1e-12 if tag == "f64" else 2e-5)
    # steps = 3 equals three calls
    ws, ds = w0, dW
    for _ in range(3):
        ws, ds = op.tangent_bundle_step(ws, ds, dt, 1)
    assert torch.equal(ws, w1) and torch.equal(ds, d1)
    # every sample of the batch equals its run alone
    for b in range(B):
        wa, da = op.tangent_bundle_step(w0[b:b + 1], dW[:, b:b + 1], dt, 3)
        assert torch.equal(wa[0], w1[b]) and torch.equal(da[:, 0], d1[:, b]), b


def test_several_chunks_per_call_equal_the_samples_alone(dev):
    """512^2 fp64, K = 2, B = 11: the chunk rule gives three chunks of 4, 4 and 3 states (16 seven-field working sets fit the
    cache, 5 states with their 2 tangents each).  Every sample carries the bits of its run alone."""
    n, B, K = 512, 11, 2
    op = J.build_op(n, "f64", "kolmogorov", dev)
    w0, dW = on(dev, *BO.inputs(n, "f64", B, K))
    plan = op._plan(w0)
    per = ctypes.c_long(0)
    plan.lib.tcfd_ns2d_plan_chunking(plan.handle, 10 ** 6, ctypes.byref(per), None, None)
    limit = per.value // (K + 1)                       # states per chunk the rule allows; a call balances its chunks below it
    nchunks = -(-B // limit)
    chunk = -(-B // nchunks)
    assert nchunks >= 3 and B % chunk != 0, f"meant to run as 4 + 4 + 3, got {nchunks} chunks of {chunk}"
    dt = J.dt_of(n)
    w1, d1 = op.tangent_bundle_step(w0, dW, dt, 1)
    f1, df1 = op.explicit_terms_jvp_bundle(w0, dW)
    for b in range(B):
        wa, da = op.tangent_bundle_step(w0[b:b + 1], dW[:, b:b + 1], dt, 1)
        fa, dfa = op.explicit_terms_jvp_bundle(w0[b:b + 1], dW[:, b:b + 1])
        assert torch.equal(wa[0], w1[b]) and torch.equal(da[:, 0], d1[:, b]), b
        assert torch.equal(fa[0], f1[b]) and torch.equal(dfa[:, 0], df1[:, b]), b
    assert rel_l2(w1, op(w0, dt, 1)[0]) <= 1e-12


# ----------------------------------------------------------------------------- shapes, the QR on the device
def test_input_shapes(dev):
    op = J.build_op(64, "f64", "kolmogorov", dev)
    w0, dW = on(dev, *BO.inputs(64, "f64", 4, 2))
    w, d = op.tangent_bundle_step(w0, dW, 1e-3, 2)
    w1, d1 = op.tangent_bundle_step(w0[0], dW[:, 0], 1e-3, 2)
    assert w1.shape == (64, 33) and d1.shape == (2, 64, 33) and torch.equal(w1, w[0]) and torch.equal(d1, d[:, 0])
    w4, d4 = op.tangent_bundle_step(w0.reshape(2, 2, 64, 33), dW.reshape(2, 2, 2, 64, 33), 1e-3, 2)
    assert w4.shape == (2, 2, 64, 33) and d4.shape == (2, 2, 2, 64, 33)
    assert torch.equal(w4.reshape(4, 64, 33), w) and torch.equal(d4.reshape(2, 4, 64, 33), d)
    f4, df4 = op.explicit_terms_jvp_bundle(w0.reshape(2, 2, 64, 33), dW.reshape(2, 2, 2, 64, 33))
    assert df4.shape == (2, 2, 2, 64, 33) and torch.equal(df4.reshape(2, 4, 64, 33), op.explicit_terms_jvp_bundle(w0, dW)[1])
    we, de = op.tangent_bundle_step(w0[:0], dW[:, :0], 1e-3)
    assert we.shape == (0, 64, 33) and de.shape == (2, 0, 64, 33)
    # a non-contiguous bundle (members taken from a larger one) is what the contiguous copy gives
    w2, d2 = op.tangent_bundle_step(w0, dW.flip(0)[::1].transpose(0, 1).contiguous().transpose(0, 1), 1e-3, 2)
    assert torch.equal(d2.flip(0), d) and torch.equal(w2, w)


def test_benettin_step_on_the_device(dev):
    """tangent_bundle_step + orthonormalize_tangents as the example uses them (64^2 fp64, K = 4): Q stays orthonormal in physical
    space to 1e-12 on the device, Q R is the stepped bundle, and the leading exponent's estimate after a few rounds is finite."""
    import torch_cfd_amd as tc

    n, K = 64, 4
    op = J.build_op(n, "f64", "kolmogorov", dev)
    w0, dW = on(dev, *BO.inputs(n, "f64", 1, K))
    Q, _ = tc.orthonormalize_tangents(dW, n)
    acc = torch.zeros(1, K, dtype=torch.float64, device=dev)
    w = w0
    for _ in range(3):
        w, dQ = op.tangent_bundle_step(w, Q, 1e-3, 5)
        Q, R = tc.orthonormalize_tangents(dQ, n)
        assert rel_l2(torch.einsum("jbxy,bjk->kbxy", Q, R.to(Q.dtype)), dQ) <= 1e-12
        acc += torch.log(torch.diagonal(R, dim1=-2, dim2=-1))
    q = torch.fft.irfft2(Q, s=(n, n))
    gram = torch.einsum("jbxy,kbxy->bjk", q, q)
    assert (gram - torch.eye(K, dtype=torch.float64, device=dev)).abs().max() <= 1e-12
    assert torch.isfinite(acc).all() and (torch.diagonal(R, dim1=-2, dim2=-1) > 0).all()


# ----------------------------------------------------------------------------- the C ABI: sizes, refusals, memory contract
def test_workspace_grows_with_tangents_and_batch(dev):
    """tcfd_ns2d_bundle_workspace_bytes never shrinks when K or the batch grows (so one buffer sized for the largest bundle serves
    every smaller one), at a size that chunks (512 fp64), one that groups (1024 fp64) and a small one; bad arguments give 0."""
    for n, tag in ((64, "f32"), (512, "f64"), (1024, "f64")):
        op = J.build_op(n, tag, "kolmogorov", dev)
        plan = op._plan(torch.zeros(1, n, n // 2 + 1, dtype=J.CPLX[tag], device=dev))
        size = lambda b, k: plan.lib.tcfd_ns2d_bundle_workspace_bytes(plan.handle, b, k)
        table = [[size(b, k) for k in range(1, 20)] for b in range(1, 24)]
        assert all(v > 0 for row in table for v in row)
        assert all(row[i] <= row[i + 1] for row in table for i in range(len(row) - 1)), (n, tag, "not monotone in K")
        assert all(table[i][k] <= table[i + 1][k] for i in range(len(table) - 1) for k in range(19)), (n, tag, "not monotone in batch")
        assert table[0][18] > table[0][0] and size(10 ** 5, 2) == size(10 ** 6, 2)       # grows with K, stops growing at one chunk
        assert size(0, 3) == 0 and size(-1, 3) == 0 and size(4, 0) == 0 and size(4, -2) == 0 and size(4, 65536) == 0


def test_c_entry_points_refuse_bad_arguments_and_ensemble_plans(dev):
    import torch_cfd_amd as tc

    n, B, K = 64, 2, 3
    op = J.build_op(n, "f64", "kolmogorov", dev)
    w0, dW = on(dev, *BO.inputs(n, "f64", B, K))
    plan, lib = op._plan(w0), tc._lib.load()
    need = lib.tcfd_ns2d_bundle_workspace_bytes(plan.handle, B, K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out, dout = torch.empty_like(w0), torch.empty_like(dW)
    one = tc._lib.darray([1.0])
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def step(w_in, dw_in, w_out, dw_out, batch=B, k=K, nbytes=need, steps=1, nst=1):
        return lib.tcfd_ns2d_step_jvp_bundle(plan.handle, w_in, dw_in, w_out, dw_out, batch, k, nst, None, one, one, one, None, None,
                                             steps, ws.data_ptr(), nbytes, st)

    def explicit(w, dw, f, df, batch=B, k=K, nbytes=need):
        return lib.tcfd_ns2d_explicit_terms_jvp_bundle(plan.handle, w, dw, f, df, batch, k, ws.data_ptr(), nbytes, st)

    P = lambda t: t.data_ptr()
    assert step(P(w0), P(dW), P(out), P(dout)) == 0 and explicit(P(w0), P(dW), None, P(dout)) == 0
    einval = lambda rc, word: rc == TCFD_EINVAL and word in lib.tcfd_last_error().decode()
    assert einval(step(P(w0), P(dW), P(out), P(dout), k=0), "ntangents") and einval(explicit(P(w0), P(dW), None, P(dout), k=0), "ntangents")
    assert einval(step(None, P(dW), P(out), P(dout)), "null") and einval(explicit(P(w0), P(dW), P(out), None), "bad argument")
    assert einval(step(P(w0), P(dW), P(out), P(dout), batch=0), "> 0") and einval(step(P(w0), P(dW), P(out), P(dout), steps=0), "> 0")
    assert einval(step(P(w0), P(dW), P(out), P(dout), nst=0), "> 0")
    # overlapping state and tangent arrays, shifted in-place outputs
    esz = w0[0].numel() * w0.element_size()
    assert einval(step(P(w0), P(dW), P(dW) + esz, P(dout)), "overlap") and einval(step(P(w0), P(dW), P(out), P(w0)), "overlap")
    assert einval(step(P(dW), P(dW), P(out), P(dout)), "overlap") and einval(step(P(w0), P(dW), P(out), P(dW) + esz), "overlap")
    assert einval(explicit(P(w0), P(dW), P(out), P(dW)), "overlap") and einval(explicit(P(w0), P(dW), P(w0), P(dout)), "overlap")
    assert step(P(w0.clone()), P(dW), P(out), P(dout)) == 0
    # a short workspace: both numbers
    for rc in (step(P(w0), P(dW), P(out), P(dout), nbytes=need - 1), explicit(P(w0), P(dW), P(out), P(dout), nbytes=need - 1)):
        msg = lib.tcfd_last_error().decode()
        assert rc == TCFD_EWORKSPACE and re.search(rf"workspace {need - 1} B < required {need} B", msg), msg
    # an ensemble plan: the refusal of the tangent-linear entry points
    torch.set_default_dtype(torch.float64)
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    ens = tc.NavierStokes2DSpectral([1e-3, 2e-3], grid, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    eplan = ens._plan(w0)
    for name, call in (("step_jvp_bundle", lambda: eplan.step_jvp_bundle(w0, dW, [0.0], [1e-3], [5e-4], 1)),
                       ("explicit_terms_jvp_bundle", lambda: eplan.explicit_terms_jvp_bundle(w0, dW))):
        with pytest.raises(tc._lib.TcfdError, match=name + r".*per-sample parameters.*one linear-term table"):
            call()
    for call in (lambda: ens.tangent_bundle_step(w0, dW, 1e-3), lambda: ens.explicit_terms_jvp_bundle(w0, dW)):
        with pytest.raises(NotImplementedError, match="per-sample parameters"):
            call()
    # the other limits of the tangent-linear step, with its messages
    with pytest.raises(NotImplementedError, match="trainable"):
        J.build_op(n, "f64", "kolmogorov", dev, solver=tc.RK4CrankNicolsonStepper(requires_grad=True)).tangent_bundle_step(w0, dW, 1e-3)
    w48 = torch.fft.rfft2(torch.randn(2, 48, 48, dtype=torch.float64)).to(dev)
    for call in (lambda o: o.tangent_bundle_step(w48, torch.stack([w48, w48]), 1e-3), lambda o: o.explicit_terms_jvp_bundle(w48, w48[None])):
        with pytest.raises(NotImplementedError, match="fused grid sizes"):
            call(J.build_op(48, "f64", "none", dev))

    class Foreign:
        def __call__(self, u, dt, equation):
            return u

    with pytest.raises(NotImplementedError, match="foreign solver"):
        J.build_op(n, "f64", "kolmogorov", dev, solver=Foreign()).tangent_bundle_step(w0, dW, 1e-3)


@pytest.mark.parametrize("n,tag,batch,K", [(8, "f64", 5, 2), (64, "f32", 3, 3), (80, "f64", 2, 2), (96, "f32", 2, 2),
                                            (512, "f64", 7, 2), (1024, "f64", 2, 4)])
def test_memory_contract(n, tag, batch, K):
    """The two entry points through guard_ops.run_guarded with the protocol of tests/test_memory_contract_gpu.py: inputs come back
    unchanged, nothing is written outside the outputs and the workspace, every output element is written, the bits do not depend
    on the poison or a dirty workspace and equal the wrapper's, the call works with exactly tcfd_ns2d_bundle_workspace_bytes and
    refuses one byte less untouched.  Bundle kernel and fall-back (80 fp64), chunks with a short last one (512 x 7 = 4 + 3),
    tangent groups (1024 fp64, K = 4), out_f = NULL, RK4-CN and the order-2 schedule (base0), in place."""
    import test_memory_contract_gpu as M
    from guard_ops import Out

    s, lib = M.ns(n, tag, batch), M._L()
    B = s.batch
    dW = M.w_hat(n, K * B, tag, seed0=7).reshape(K, B, n, s.m) * 0.25
    need = lib.tcfd_ns2d_bundle_workspace_bytes(s.h, B, K)
    assert need > 0 and lib.tcfd_ns2d_bundle_workspace_bytes(s.h, 0, K) == 0
    touts = lambda: Out(s.cdt, (K,) + s.shape)
    ins = {"w": s.w, "dw": dW}
    f, df = s.plan.explicit_terms_jvp_bundle(s.w, dW)
    M.guard("tcfd_ns2d_explicit_terms_jvp_bundle", ins, {"f": s.out(), "df": touts()},
            lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_jvp_bundle(s.h, P("w"), P("dw"), P("f"), P("df"), B, K, ws, nb, M._stream()),
            need, {"f": f, "df": df})
    M.guard("tcfd_ns2d_explicit_terms_jvp_bundle out_f=NULL", ins, {"df": touts()},
            lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_jvp_bundle(s.h, P("w"), P("dw"), None, P("df"), B, K, ws, nb, M._stream()),
            need, {"df": df})
    for sc in (s.op._schedule(s.op.solver, s.op.solver.params, s.dt), s.imex2.stage_schedule(s.imex2.params, s.dt)):
        beta, gdt, mu, nst = sc["beta"], sc["gdt"], sc["mu"], len(sc["beta"])
        ints = (ctypes.c_int * nst)(*[int(v) for v in sc["base0"]]) if sc["base0"] is not None else None
        ref = s.plan.step_jvp_bundle(s.w, dW, beta, gdt, mu, 2, fa=sc["fa"], mu_den=sc["mu_den"], base0=sc["base0"])

        def call(P, wo, dwo, ws, nb):
            return lib.tcfd_ns2d_step_jvp_bundle(s.h, P("w"), P("dw"), P(wo), P(dwo), B, K, nst, M._darr(sc["fa"]), M._darr(beta),
                                                 M._darr(gdt), M._darr(mu), M._darr(sc["mu_den"]), ints, 2, ws, nb, M._stream())

        M.guard(f"tcfd_ns2d_step_jvp_bundle nstages={nst}", ins, {"wo": s.out(), "dwo": touts()},
                lambda P, ws, nb: call(P, "wo", "dwo", ws, nb), need, {"wo": ref[0], "dwo": ref[1]})
        M.guard(f"tcfd_ns2d_step_jvp_bundle nstages={nst} in place", ins, {"w": s.out(), "dw": touts()},
                lambda P, ws, nb: call(P, "w", "dw", ws, nb), need, {"w": ref[0], "dw": ref[1]})
    if n >= 1024:
        M.ns.cache_clear()     # the large plan and its inputs do not outlive the case
        torch.cuda.empty_cache()
