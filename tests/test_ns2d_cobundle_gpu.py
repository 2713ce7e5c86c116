"""K cotangents per trajectory in one adjoint call on the device (tcfd_ns2d_explicit_terms_vjp_bundle / tcfd_ns2d_step_vjp_bundle,
k_rows_vjp_bundle and the out-of-place fall-back k_rows_vjp_oop): NavierStokes2DSpectral.adjoint_bundle_step.

References: the CPU stepper in fp64 under torch autograd, one forward evaluation per bundle (ns2d_cobundle_ops.oracle_cobundle,
tied to the goldens made from the reference by tests/test_ns2d_cobundle_host.py); the single-cotangent calls of the same build;
the tangent bundle.  Bounds are the project's (tests/test_ns2d_bundle_gpu.py, tests/test_ns2d_step_vjp_gpu.py): the explicit
terms' cotangents 1e-10 (fp64) / 2e-5 (fp32) relative L2 against the fp64 reference, stepped cotangents 1e-9 / 2e-5, member k
against adjoint_step alone 1e-12 / 2e-5 (whether the bits are equal is printed), the adjoint identity 1e-12 / 1e-5 of
|J dW_i| |G_j|.  Independence, homogeneity, checkpointing, chunking and reproducibility are compared bitwise.

Sizes: 8 (smallest plan), 16, 64; 80 (fp64: fall-back, fp32: 20 elements per lane in the bundle kernel), 96 (12 per lane), 1024
(workgroup-wide transforms; fp64 with K = 4: one state per chunk, cotangent groups of 2), 1536 (fp64: fall-back by the LDS rule),
512 x 11 (fp32: two chunks of 6 and 5; fp64: three chunks of 4, 4 and 3 -- the last one short either way).
"""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import ns2d_bundle_ops as BO
import ns2d_cobundle_ops as CO
import ns2d_ops
import ns2d_step_vjp_ops as V
import test_ns2d_jvp_gpu as J
from conftest import rel_l2

pytestmark = pytest.mark.gpu

L = 2 * math.pi
IMEX = J.IMEX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _plan(op, like):
    return op._plan(like)


# ----------------------------------------------------------------------------- 1. explicit terms' VJP against the CPU reference
EXPLICIT_CASES = [(n, tag, 2, 3) for n in (8, 16, 64, 80, 96) for tag in ("f64", "f32")] + [
    (1024, "f64", 1, 2), (1024, "f32", 1, 2), (1536, "f64", 1, 2)]


@functools.lru_cache(maxsize=None)
def explicit_reference(n, tag, B, K):
    from oracle import ns2d as O

    w0, G = CO.inputs(n, tag, B, K)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        t = ns2d_ops.tables(n, "kolmogorov", True).oracle
        return CO.oracle_cobundle(lambda w: O.explicit_terms(w, t), w0.to(torch.complex128), G.to(torch.complex128))[1]
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("n,tag,B,K", EXPLICIT_CASES)
def test_explicit_terms_vjp_bundle_against_cpu_reverse_mode(n, tag, B, K, dev):
    """wbar_k = sum_f post_f X_f of the bundle call against autograd through the fp64 oracle: 1e-10 (fp64), 2e-5 (fp32); then
    member k against explicit_terms_vjp alone (1e-12 / 2e-5; bits printed), and K = 1."""
    ref = explicit_reference(n, tag, B, K)
    w0, G = on(dev, *CO.inputs(n, tag, B, K))
    op = J.build_op(n, tag, "kolmogorov", dev)
    plan = _plan(op, w0)
    GM, post = CO.pre_weighted(op, plan, G)
    tol, tol_m = (1e-10, 1e-12) if tag == "f64" else (2e-5, 2e-5)
    X = plan.explicit_terms_vjp_bundle(w0, GM)
    assert X.shape == (K, 4, B, n, n // 2 + 1) and X.dtype == w0.dtype
    wbar = (post[None, :, None] * X).sum(1)
    errs = [rel_l2(wbar[k], ref[k]) for k in range(K)]
    print(f"n={n} {tag} B={B} K={K}: wbar " + " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= tol
    for k in range(K):
        X1 = plan.explicit_terms_vjp(w0, GM[k])
        e = rel_l2(X[k], X1)
        print(f"  member {k} against explicit_terms_vjp alone: {e:.3e} bits equal: {torch.equal(X[k], X1)}")
        assert e <= tol_m
        assert torch.equal(plan.explicit_terms_vjp_bundle(w0, GM[k:k + 1])[0], X[k])          # K = 1


# ----------------------------------------------------------------------------- 2. stepped bundle against the CPU reference
@functools.lru_cache(maxsize=None)
def stepped_reference(n, tag, forcing, smooth):
    """fp64 references from the (possibly fp32) inputs, B = 2, K = 3: RK4-CN at 1 and 3 steps from the oracle's own stepper, the
    IMEX orders (2 steps) from the stage loop of tests/ns2d_ops.py on the package's schedules."""
    import torch_cfd_amd as tc
    from oracle import ns2d as O

    w0, G = CO.inputs(n, tag, 2, 3)
    w64, g64 = w0.to(torch.complex128), G.to(torch.complex128)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        t = ns2d_ops.tables(n, forcing, smooth)
        out = {}
        for steps in (1, 3):
            out[f"rk{steps}"] = CO.oracle_cobundle(lambda w: O.advance(w, J.dt_of(n), t.oracle, steps=steps)[0], w64, g64)
        for name, (order, alpha, beta) in IMEX.items():
            sched = ns2d_ops.schedule(tc.IMEXStepper(order=order, alpha=alpha, beta=beta), J.dt_of(n))
            out[name] = CO.oracle_cobundle(lambda w: ns2d_ops.advance(w, t, sched, 2), w64, g64)
        return out
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", ["kolmogorov", "none"])
@pytest.mark.parametrize("n", [16, 64])
def test_stepped_bundle_against_cpu_reverse_mode(n, forcing, smooth, tag, dev):
    """RK4-CN for 1 and 3 steps and IMEX orders 1, 1.5, 2 (2 steps; order 2 restarts its second stage from the step's initial
    state), forcing and `smooth` on and off: cotangents 1e-9 / 2e-5 against the fp64 reference, member k against
    adjoint_step(w, G[k]) 1e-12 / 2e-5, and w_new bit-equal to op(w, dt, steps)[0]."""
    import torch_cfd_amd as tc

    ref = stepped_reference(n, tag, forcing, smooth)
    w0, G = on(dev, *CO.inputs(n, tag, 2, 3))
    dt = J.dt_of(n)
    tol, tol_m = (1e-9, 1e-12) if tag == "f64" else (2e-5, 2e-5)
    cases = [(f"rk{s}", None, s) for s in (1, 3)] + [(name, tc.IMEXStepper(order=o, alpha=a, beta=b), 2) for name, (o, a, b) in IMEX.items()]
    for name, stepper, steps in cases:
        op = J.build_op(n, tag, forcing, dev, smooth, solver=stepper)
        w, Wbar = op.adjoint_bundle_step(w0, G, dt, steps)
        e_c = max(rel_l2(Wbar[k], ref[name][1][k]) for k in range(3))
        e_m = max(rel_l2(Wbar[k], op.adjoint_step(w0, G[k], dt, steps)[1]) for k in range(3))
        print(f"n={n} {tag} {forcing} smooth={smooth} {name}: cotangents {e_c:.3e} against adjoint_step alone {e_m:.3e}")
        assert Wbar.shape == G.shape and e_c <= tol and e_m <= tol_m, name
        assert torch.equal(w, op(w0, dt, steps)[0]), name


# ----------------------------------------------------------------------------- 3. adjoint identity with the tangent bundle
@pytest.mark.parametrize("n,tag", [(64, "f64"), (64, "f32"), (96, "f64"), (96, "f32")])
def test_adjoint_identity_with_the_tangent_bundle_all_pairs(n, tag, dev):
    """<J dW_i, G_j> = <dW_i, Wbar_j> in the real inner product for the K x K matrix, J dW from tangent_bundle_step, Wbar from
    adjoint_bundle_step, B = 1, K = 3, two steps: 1e-12 (fp64) / 1e-5 (fp32) of |J dW_i| |G_j|."""
    K = 3
    w0, dW = on(dev, *BO.inputs(n, tag, 1, K))
    _, G = on(dev, *CO.inputs(n, tag, 1, K))
    op = J.build_op(n, tag, "kolmogorov", dev)
    dt, steps = J.dt_of(n), 2
    tol = 1e-12 if tag == "f64" else 1e-5
    _, JdW = op.tangent_bundle_step(w0, dW, dt, steps)
    _, Wbar = op.adjoint_bundle_step(w0, G, dt, steps)
    for i in range(K):
        for j in range(K):
            lhs, rhs = ns2d_ops.real_inner(JdW[i], G[j]).item(), ns2d_ops.real_inner(dW[i], Wbar[j]).item()
            scale = (torch.linalg.norm(JdW[i]) * torch.linalg.norm(G[j])).item()
            print(f"n={n} {tag} ({i}, {j}): <JdW,G> {lhs:.12e} <dW,Wbar> {rhs:.12e} defect/scale {abs(lhs - rhs) / scale:.3e}")
            assert abs(lhs - rhs) <= tol * scale, (i, j)


# ----------------------------------------------------------------------------- 4. the whole transposed Jacobian at n = 8
def test_whole_transposed_jacobian_n8(dev):
    """n = 8, fp64, one RK4-CN step: dW = rfft2 of the 64 real-space unit fields, G the same, K = 64 in both calls.  The 64 x 64
    matrices <J dW_i, G_j> and <dW_i, Wbar_j> agree to 1e-12 of the largest entry -- this reaches the ky = 0 and Nyquist columns
    and the mask's edge, which random vectors under-weight."""
    n = 8
    op = J.build_op(n, "f64", "kolmogorov", dev)
    w0 = BO.inputs(n, "f64", 1, 1)[0][0].to(dev)
    E = torch.fft.rfft2(torch.eye(n * n, dtype=torch.float64).reshape(n * n, n, n)).to(dev)
    _, JE = op.tangent_bundle_step(w0, E, 1e-3, 1)
    _, Wbar = op.adjoint_bundle_step(w0, E, 1e-3, 1)
    inner = lambda A, Bm: torch.einsum("ixy,jxy->ij", A.real, Bm.real) + torch.einsum("ixy,jxy->ij", A.imag, Bm.imag)
    lhs, rhs = inner(JE, E), inner(E, Wbar)
    top = lhs.abs().max().item()
    print(f"whole Jacobian n=8: largest entry {top:.6e}, largest defect {(lhs - rhs).abs().max().item():.3e}")
    assert top > 0 and (lhs - rhs).abs().max().item() <= 1e-12 * top


# ----------------------------------------------------------------------------- 5. exact properties, bitwise
@pytest.mark.parametrize("n,tag,solver", [(64, "f64", "rk4"), (64, "f32", "imex2"), (80, "f64", "rk4"), (96, "f32", "rk4")])
def test_bundle_properties_bitwise(n, tag, solver, dev):
    import torch_cfd_amd as tc

    stepper = None if solver == "rk4" else tc.IMEXStepper(order=IMEX[solver][0], alpha=IMEX[solver][1], beta=IMEX[solver][2])
    op = J.build_op(n, tag, "kolmogorov", dev, solver=stepper)
    B, K, steps = 2, 3, 3
    w0, G = on(dev, *CO.inputs(n, tag, B, K))
    dt = J.dt_of(n)
    w1, b1 = op.adjoint_bundle_step(w0, G, dt, steps)
    # a second run gives the same bits
    w1b, b1b = op.adjoint_bundle_step(w0, G, dt, steps)
    assert torch.equal(w1, w1b) and torch.equal(b1, b1b)
    # a zero member gives exact zeros while the others keep their bits
    GZ = G.clone()
    GZ[1] = 0
    wz, bz = op.adjoint_bundle_step(w0, GZ, dt, steps)
    assert (bz[1] == 0).all() and (bz[0] != 0).any()
    assert torch.equal(bz[0], b1[0]) and torch.equal(bz[2], b1[2]) and torch.equal(wz, w1)
    # exact homogeneity (a power of two scales every intermediate exactly)
    w2, b2 = op.adjoint_bundle_step(w0, 2 * G, dt, steps)
    assert torch.equal(w2, w1) and torch.equal(b2, 2 * b1)
    # member k is unchanged when the other members are replaced, and equals the K = 1 call
    for k in range(K):
        wk, bk = op.adjoint_bundle_step(w0, G[k:k + 1], dt, steps)
        assert torch.equal(bk[0], b1[k]) and torch.equal(wk, w1), k
    wp, bp = op.adjoint_bundle_step(w0, G.flip(0), dt, steps)
    assert torch.equal(wp, w1) and torch.equal(bp.flip(0), b1)
    # checkpointing: the same bits for every segment length
    for every in (1, 2, steps):
        wc, bc = op.adjoint_bundle_step(w0, G, dt, steps, checkpoint_every=every)
        assert torch.equal(wc, w1) and torch.equal(bc, b1), every
    # steps = 3 in one call equals three calls of one step, chained (last step first)
    states = [w0]
    for _ in range(steps - 1):
        states.append(op(states[-1], dt, 1)[0])
    bs = G
    for s in reversed(range(steps)):
        _, bs = op.adjoint_bundle_step(states[s], bs, dt, 1)
    assert torch.equal(bs, b1)
    # every sample of the batch equals its run alone
    for b in range(B):
        wa, ba = op.adjoint_bundle_step(w0[b:b + 1], G[:, b:b + 1], dt, steps)
        assert torch.equal(wa[0], w1[b]) and torch.equal(ba[:, 0], b1[:, b]), b
    # g_dwdt is folded in as adjoint_step folds it
    g2 = G.flip(0).contiguous() * 0.5
    _, bd = op.adjoint_bundle_step(w0, G, dt, steps, g_dwdt=g2)
    tol = 1e-12 if tag == "f64" else 2e-5
    for k in range(K):
        assert rel_l2(bd[k], op.adjoint_step(w0, G[k], dt, steps, g_dwdt=g2[k])[1]) <= tol, k


@pytest.mark.parametrize("tag,least", [("f32", 2), ("f64", 3)])
def test_several_chunks_per_call_equal_the_samples_alone(tag, least, dev):
    """512^2, K = 2, B = 11: in fp32 the cache holds 32 seven-field working sets, 10 states with their 2 cotangents each, so the
    call runs as two chunks of 6 and 5; in fp64 16 sets, 5 states, three chunks of 4, 4 and 3.  Either way the last chunk is
    short, and every sample carries the bits of its run alone."""
    n, B, K = 512, 11, 2
    op = J.build_op(n, tag, "kolmogorov", dev)
    w0, G = on(dev, *CO.inputs(n, tag, B, K))
    plan = _plan(op, w0)
    per = ctypes.c_long(0)
    plan.lib.tcfd_ns2d_plan_chunking(plan.handle, 10 ** 6, ctypes.byref(per), None, None)
    limit = per.value // (K + 1)                       # states per chunk the rule allows; a call balances its chunks below it
    nchunks = -(-B // limit)
    chunk = -(-B // nchunks)
    print(f"512 x {B} {tag}, K = {K}: {nchunks} chunks of at most {chunk}")
    assert nchunks >= least and B % chunk != 0, f"meant to run as {least} chunks with a short last one, got {nchunks} chunks of {chunk}"
    dt = J.dt_of(n)
    w1, b1 = op.adjoint_bundle_step(w0, G, dt, 1)
    for b in range(B):
        wa, ba = op.adjoint_bundle_step(w0[b:b + 1], G[:, b:b + 1], dt, 1)
        assert torch.equal(wa[0], w1[b]) and torch.equal(ba[:, 0], b1[:, b]), b


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_fall_back_rows_against_the_bundle_kernel(tag, dev, monkeypatch):
    """TCFD_BUNDLE_ROWS=0 (k_rows_vjp_oop once per cotangent at every size) against the default at n = 64: 1e-12 / 2e-5.  Which
    row kernel ran is read off the library's launch records: one row-pass launch for the K = 3 cotangents of one sweep by
    default, three under the switch."""
    n, B, K = 64, 2, 3
    w0, G = on(dev, *CO.inputs(n, tag, B, K))
    dt = J.dt_of(n)
    op1 = J.build_op(n, tag, "kolmogorov", dev)
    _, c1 = op1.adjoint_bundle_step(w0, G, dt, 2)
    monkeypatch.setenv("TCFD_BUNDLE_ROWS", "0")          # read once, when the plan is created: a second operator
    op0 = J.build_op(n, tag, "kolmogorov", dev)
    _, c0 = op0.adjoint_bundle_step(w0, G, dt, 2)
    monkeypatch.delenv("TCFD_BUNDLE_ROWS")
    launches = [CO.row_launches(_plan(o, w0), lambda o=o: _plan(o, w0).explicit_terms_vjp_bundle(w0, G)) for o in (op1, op0)]
    print(f"n={n} {tag}: row-pass launches of one sweep, default {launches[0]}, TCFD_BUNDLE_ROWS=0 {launches[1]}")
    assert launches == [1, K]
    e = rel_l2(c0, c1)
    print(f"n={n} {tag}: fall-back against the bundle kernel {e:.3e}, bits equal: {torch.equal(c0, c1)}")
    assert (c1 != 0).any() and e <= (1e-12 if tag == "f64" else 2e-5)


# ----------------------------------------------------------------------------- 6. grouping
def test_cotangent_groups_at_1024_fp64(dev):
    """1024^2 fp64, B = 2, K = 4: the cache holds 4 seven-field working sets, so a chunk is ONE state and its cotangents pass in
    groups (limit 3, balanced to 2 + 2).  The shape is read off the workspace size, which is cobundle_fields(K, 3, nstages) fields
    of a one-state chunk; the result agrees with K separate adjoint_step calls to 1e-12."""
    n, B, K = 1024, 2, 4
    op = J.build_op(n, "f64", "kolmogorov", dev)
    w0, G = on(dev, *CO.inputs(n, "f64", B, K))
    plan = _plan(op, w0)
    per = ctypes.c_long(0)
    plan.lib.tcfd_ns2d_plan_chunking(plan.handle, 10 ** 6, ctypes.byref(per), None, None)
    cap = per.value
    assert 2 <= cap < K + 1, f"meant to group: {cap} working sets fit the cache"
    field = plan.lib.tcfd_ns2d_workspace_bytes(plan.handle, 1) // 8                      # one chunk-sized field of a one-state chunk
    nst = 4
    need = plan.lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes(plan.handle, B, K, nst)
    assert need == (7 + nst + 9 * (cap - 1) + 4 * K) * field, (need, field, cap)
    # ... and the launch records show the two groups: two row-pass launches for the four cotangents of one state's sweep
    assert CO.row_launches(plan, lambda: plan.explicit_terms_vjp_bundle(w0[:1], G[:, :1].contiguous())) == 2
    dt = J.dt_of(n)
    w1, b1 = op.adjoint_bundle_step(w0, G, dt, 1)
    for k in range(K):
        e = rel_l2(b1[k], op.adjoint_step(w0, G[k], dt, 1)[1])
        print(f"1024 fp64 K=4 member {k} against adjoint_step alone: {e:.3e}")
        assert e <= 1e-12, k
    assert torch.equal(w1, op(w0, dt, 1)[0])


# ----------------------------------------------------------------------------- 7. the C ABI: sizes, refusals, memory contract
def test_workspace_grows_with_cotangents_and_batch(dev):
    """tcfd_ns2d_step_vjp_bundle_workspace_bytes never shrinks when K or the batch grows, at a size that chunks (512 fp64), one
    that groups (1024 fp64) and a small one; bad arguments give 0."""
    for n, tag in ((64, "f32"), (512, "f64"), (1024, "f64")):
        op = J.build_op(n, tag, "kolmogorov", dev)
        plan = _plan(op, torch.zeros(1, n, n // 2 + 1, dtype=J.CPLX[tag], device=dev))
        size = lambda b, k, s=4: plan.lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes(plan.handle, b, k, s)
        table = [[size(b, k) for k in range(1, 20)] for b in range(1, 24)]
        assert all(v > 0 for row in table for v in row)
        assert all(row[i] <= row[i + 1] for row in table for i in range(len(row) - 1)), (n, tag, "not monotone in K")
        assert all(table[i][k] <= table[i + 1][k] for i in range(len(table) - 1) for k in range(19)), (n, tag, "not monotone in batch")
        assert table[0][18] > table[0][0] and size(10 ** 5, 2) == size(10 ** 6, 2)       # grows with K, stops growing at one chunk
        assert size(2, 3, 5) > size(2, 3, 4)
        assert size(0, 3) == 0 and size(-1, 3) == 0 and size(4, 0) == 0 and size(4, -2) == 0 and size(4, 65536) == 0
        assert size(4, 3, 0) == 0 and size(4, 3, 33) == 0


def test_c_entry_points_refuse_bad_arguments_and_ensemble_plans(dev):
    import torch_cfd_amd as tc
    from torch_cfd_amd.autograd import FusedExplicitTerms

    n, B, K = 64, 2, 3
    op = J.build_op(n, "f64", "kolmogorov", dev)
    w0, G = on(dev, *CO.inputs(n, "f64", B, K))
    plan, lib = _plan(op, w0), tc._lib.load()
    pre, post = FusedExplicitTerms._tables(op, plan, dev)
    need = lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes(plan.handle, B, K, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    saved = torch.stack([w0, w0 * 0.5]).contiguous()
    gin, X = torch.empty_like(G), torch.empty((K, 4) + tuple(w0.shape), dtype=w0.dtype, device=dev)
    one = tc._lib.darray([1.0])
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: t.data_ptr()

    def step(sv, g_out, g_in, batch=B, k=K, nbytes=need, steps=2, nst=1, pre_=P(pre)):
        return lib.tcfd_ns2d_step_vjp_bundle(plan.handle, sv, g_out, pre_, P(post), g_in, batch, k, nst, None, one, one, one, None,
                                             None, steps, ws.data_ptr(), nbytes, st)

    def explicit(w, gm, x, batch=B, k=K, nbytes=need):
        return lib.tcfd_ns2d_explicit_terms_vjp_bundle(plan.handle, w, gm, x, batch, k, ws.data_ptr(), nbytes, st)

    assert step(P(saved), P(G), P(gin)) == 0 and explicit(P(w0), P(G), P(X)) == 0
    einval = lambda rc, word: rc == TCFD_EINVAL and word in lib.tcfd_last_error().decode()
    assert einval(step(P(saved), P(G), P(gin), k=0), "ncotangents") and einval(step(P(saved), P(G), P(gin), k=65536), "ncotangents")
    assert einval(explicit(P(w0), P(G), P(X), k=0), "ncotangents")
    assert einval(step(None, P(G), P(gin)), "null") and einval(step(P(saved), P(G), None), "null")
    assert einval(step(P(saved), P(G), P(gin), pre_=None), "null") and einval(explicit(P(w0), None, P(X)), "null")
    assert einval(step(P(saved), P(G), P(gin), batch=0), "batch") and einval(step(P(saved), P(G), P(gin), steps=0), "steps")
    assert einval(step(P(saved), P(G), P(gin), nst=0), "nstages") and einval(step(P(saved), P(G), P(gin), nst=33), "nstages")
    assert einval(step(P(saved), P(G), P(gin), batch=2 ** 24, k=65535), "largest batch")
    # g_in over the saved states, g_in shifted against g_out, xout over an input
    esz = w0[0].numel() * w0.element_size()
    assert einval(step(P(saved), P(G), P(saved) + esz), "overlaps saved")
    assert einval(step(P(saved), P(G), P(G) + esz), "overlaps g_out")
    assert einval(explicit(P(w0), P(G), P(G)), "overlap") and einval(explicit(P(w0), P(G), P(w0)), "overlap")
    assert step(P(saved), P(G.clone()), P(gin)) == 0
    # a short workspace: both numbers
    for rc in (step(P(saved), P(G), P(gin), nbytes=need - 1), explicit(P(w0), P(G), P(X), nbytes=need - 1)):
        msg = lib.tcfd_last_error().decode()
        assert rc == TCFD_EWORKSPACE and re.search(rf"workspace {need - 1} B < required {need} B", msg), msg
    # an ensemble plan
    torch.set_default_dtype(torch.float64)
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    ens = tc.NavierStokes2DSpectral([1e-3, 2e-3], grid, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    eplan = ens._plan(w0)
    for name, call in (("step_vjp_bundle", lambda: eplan.step_vjp_bundle(saved, G, pre, post, [0.0], [1e-3], [5e-4])),
                       ("explicit_terms_vjp_bundle", lambda: eplan.explicit_terms_vjp_bundle(w0, G))):
        with pytest.raises(tc._lib.TcfdError, match=name + r".*per-sample parameters"):
            call()
    with pytest.raises(NotImplementedError, match="per-sample parameters"):
        ens.adjoint_bundle_step(w0, G, 1e-3)
    # the other limits of the adjoint model, with its messages
    with pytest.raises(NotImplementedError, match="trainable"):
        J.build_op(n, "f64", "kolmogorov", dev, solver=tc.RK4CrankNicolsonStepper(requires_grad=True)).adjoint_bundle_step(w0, G, 1e-3)
    w48 = torch.fft.rfft2(torch.randn(2, 48, 48, dtype=torch.float64)).to(dev)
    with pytest.raises(NotImplementedError, match="fused grid sizes"):
        J.build_op(48, "f64", "none", dev).adjoint_bundle_step(w48, torch.stack([w48, w48]), 1e-3)

    class Foreign:
        def __call__(self, u, dt, equation):
            return u

    with pytest.raises(NotImplementedError, match="foreign solver"):
        J.build_op(n, "f64", "kolmogorov", dev, solver=Foreign()).adjoint_bundle_step(w0, G, 1e-3)


@pytest.mark.parametrize("n,tag,batch,K", [(8, "f64", 5, 2), (64, "f32", 3, 3), (80, "f64", 2, 2), (96, "f32", 2, 2),
                                            (512, "f64", 7, 2), (1024, "f64", 2, 4)])
def test_memory_contract(n, tag, batch, K):
    """The two entry points through guard_ops.run_guarded with the protocol of tests/test_memory_contract_gpu.py: saved, g_out, pre
    and post come back unchanged, nothing is written outside g_in (xout) and the workspace, every output element is written, the
    bits do not depend on the poison or a dirty workspace and equal the wrapper's, the call works with exactly
    tcfd_ns2d_step_vjp_bundle_workspace_bytes and refuses one byte less untouched.  Bundle kernel and fall-back (80 fp64), chunks
    with a short last one (512 x 7), cotangent groups (1024 fp64, K = 4), RK4-CN and the order-2 schedule (base0), in place."""
    import test_memory_contract_gpu as M
    from guard_ops import Out
    from torch_cfd_amd.autograd import FusedExplicitTerms

    s, lib = M.ns(n, tag, batch), M._L()
    B = s.batch
    G = M.w_hat(n, K * B, tag, seed0=7).reshape(K, B, n, s.m) * 0.25
    pre, post = FusedExplicitTerms._tables(s.op, s.plan, M._dev())
    couts = lambda: Out(s.cdt, (K,) + s.shape)
    need1 = lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes(s.h, B, K, 1)
    assert need1 > 0 and lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes(s.h, 0, K, 1) == 0
    X = s.plan.explicit_terms_vjp_bundle(s.w, G)
    M.guard("tcfd_ns2d_explicit_terms_vjp_bundle", {"w": s.w, "gm": G}, {"x": Out(s.cdt, (K, 4) + s.shape)},
            lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_vjp_bundle(s.h, P("w"), P("gm"), P("x"), B, K, ws, nb, M._stream()),
            need1, {"x": X})
    for sc in (s.op._schedule(s.op.solver, s.op.solver.params, s.dt), s.imex2.stage_schedule(s.imex2.params, s.dt)):
        beta, gdt, mu, nst = sc["beta"], sc["gdt"], sc["mu"], len(sc["beta"])
        ints = (ctypes.c_int * nst)(*[int(v) for v in sc["base0"]]) if sc["base0"] is not None else None
        need = lib.tcfd_ns2d_step_vjp_bundle_workspace_bytes(s.h, B, K, nst)
        kw = dict(fa=sc["fa"], mu_den=sc["mu_den"], base0=sc["base0"])
        saved = torch.stack([s.w, s.plan.step(s.w, beta, gdt, mu, 1, 1.0, False, **kw)[0]]).contiguous()
        ref = s.plan.step_vjp_bundle(saved, G, pre, post, beta, gdt, mu, **kw)

        def call(P, gin, ws, nb):
            return lib.tcfd_ns2d_step_vjp_bundle(s.h, P("saved"), P("g"), P("pre"), P("post"), P(gin), B, K, nst, M._darr(sc["fa"]),
                                                 M._darr(beta), M._darr(gdt), M._darr(mu), M._darr(sc["mu_den"]), ints, 2, ws, nb,
                                                 M._stream())

        ins = {"saved": saved, "g": G, "pre": pre, "post": post}
        M.guard(f"tcfd_ns2d_step_vjp_bundle nstages={nst}", ins, {"gin": couts()}, lambda P, ws, nb: call(P, "gin", ws, nb), need,
                {"gin": ref})
        M.guard(f"tcfd_ns2d_step_vjp_bundle nstages={nst} in place", ins, {"g": couts()}, lambda P, ws, nb: call(P, "g", ws, nb), need,
                {"g": ref})
    if n >= 1024:
        M.ns.cache_clear()     # the large plan and its inputs do not outlive the case
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 8. the example
def test_singular_vector_example_runs():
    """examples/kolmogorov_singular_vectors.py at 64^2, K = 3, a short window (30 steps), in a child process: the printed
    residuals |J^T J v - sigma^2 v| / sigma^2 are below 1e-6.  The block carries 13 guard vectors: the singular values of a short
    window lie close together, and the iteration converges like (sigma_17 / sigma_3)^2 per application (with 4 guard vectors and
    10 steps the third pair was still at 1.5e-5 after 80)."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "kolmogorov_singular_vectors.py"), "--n", "64", "--k", "3", "--guard", "13",
           "--steps", "30", "--spinup", "50", "--iterations", "150", "--tol", "1e-7"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(run.stdout[-3000:], run.stderr[-2000:])
    assert run.returncode == 0
    pairs = re.findall(r"^\s+sigma\s+(\S+)\s+residual\s+(\S+)\s*$", run.stdout, flags=re.M)
    sig, res = [float(a) for a, _ in pairs], [float(b) for _, b in pairs]
    assert len(res) == 3 and len(sig) == 3 and sig == sorted(sig, reverse=True) and all(v > 0 for v in sig)
    assert max(res) < 1e-6, res
