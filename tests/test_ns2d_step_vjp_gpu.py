"""The adjoint model of the fused spectral step on the device: tcfd_ns2d_step_vjp (k_stage_adjoint, k_vjp_close around the
explicit terms' adjoint sweep), ``NavierStokes2DSpectral.adjoint_step`` and the one-node autograd path ``FusedSteps``.

References and bounds.  (1) Goldens made from the reference's own autograd (tests/golden/ns2d_step_vjp.npz, n = 16; tied to the
CPU oracle by tests/test_ns2d_step_vjp_host.py): rel-L2 over every element 1e-9 in fp64 and 2e-5 in fp32, the bounds of the
stepped tangents in tests/test_ns2d_jvp_gpu.py; the per-stage node chain (TCFD_FUSED_ADJOINT=0) is held to the same golden.
(2) The adjoint identity <J dw, g> = <dw, J^T g> with J dw from the tangent-linear kernels: 1e-12 / 1e-5 relative to |J dw| |g|,
as test_adjoint_identity_against_the_fused_vjp.  (3) The per-stage node chain: 1e-10 / 2e-5, the first-derivative bounds of
test_second_order_gradients_through_the_fused_nodes / test_fused_vjp_of_the_explicit_terms....  Reproducibility, batch
independence, checkpointing and aliasing are compared bitwise.  (5) The entry point on guarded, poisoned buffers
(tests/guard_ops.py), with the operators and the ``guard`` protocol of tests/test_memory_contract_gpu.py.
"""
import ctypes

import pytest
import torch

import ns2d_ops
import ns2d_step_vjp_ops as V
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

TCFD_EINVAL, TCFD_EWORKSPACE = -1, -4


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _tol(tag, f64, f32):
    return f64 if tag == "f64" else f32


# ----------------------------------------------------------------------------- 1. goldens from the reference (n = 16)
def _golden_case(g, prefix, tag, forcing, smooth, dev, monkeypatch, bound):
    dt = float(g["dt"])
    w0, cot = torch.from_numpy(g[prefix + "w0"]).to(dev), torch.from_numpy(g[prefix + "cot"]).to(dev)
    key = f"{prefix}{forcing}_s{int(smooth)}_"
    worst = {}
    for what, (solver, steps) in V.GOLDEN_RUNS.items():
        op = V.build_op(16, tag, forcing, dev, smooth, solver)
        want = g[key + what]
        got = {}
        for flag, name in (("1", "FusedSteps"), ("0", "per-stage nodes")):
            monkeypatch.setenv("TCFD_FUSED_ADJOINT", flag)
            got[name], node = V.grad_through_forward(op, w0, dt, steps, cot)
            assert ("FusedSteps" in node) == (flag == "1"), (node, flag)
        monkeypatch.delenv("TCFD_FUSED_ADJOINT")
        w_new, got["adjoint_step"] = op.adjoint_step(w0, cot, dt, steps)
        assert rel_l2(w_new, op(w0, dt, steps)[0]) <= _tol(tag, 1e-12, 2e-5), what
        for name, wbar in got.items():
            assert wbar.dtype == w0.dtype
            err = rel_l2(wbar, want)
            print(f"{key}{what} {name}: {err:.3e}")
            worst[name] = max(worst.get(name, 0.0), err)
    for name, err in worst.items():
        assert err <= bound, (name, err)


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("forcing", ["none", "kolmogorov"])
def test_golden_gradients_fp64(forcing, smooth, dev, monkeypatch):
    """w.grad of <cot, forward(w, dt)^K>: RK4-CN at K = 1, 3 and the three IMEX schedules at K = 2 (order 2 restarts its second
    stage from the step's initial state) -- through FusedSteps, through the per-stage node chain and from adjoint_step."""
    _golden_case(load_golden("ns2d_step_vjp.npz"), "", "f64", forcing, smooth, dev, monkeypatch, 1e-9)


def test_golden_gradients_fp32(dev, monkeypatch):
    """complex64 run against the reference's complex64 gradients (both carry fp32 round-off: 2e-5)."""
    _golden_case(load_golden("ns2d_step_vjp.npz"), "f32_", "f32", "kolmogorov", True, dev, monkeypatch, 2e-5)


# ----------------------------------------------------------------------------- 2. adjoint identity with the tangent kernels
IDENTITY_CASES = [(8, "f64", 3, "none", (1, 3)), (64, "f64", 3, "kolmogorov", (1, 3)), (64, "f32", 3, "kolmogorov", (1, 3)),
                  (80, "f64", 2, "none", (1, 3)), (96, "f32", 2, "none", (1, 3)), (256, "f64", 2, "kolmogorov", (1, 3)),
                  (512, "f64", 2, "kolmogorov", (1, 3)), (1024, "f64", 1, "none", (1, 3)), (1024, "f32", 1, "kolmogorov", (1, 3)),
                  (2048, "f64", 1, "kolmogorov", (1,))]


@pytest.mark.parametrize("n,tag,B,forcing,step_counts", IDENTITY_CASES, ids=[f"n{c[0]}-{c[1]}-b{c[2]}" for c in IDENTITY_CASES])
def test_adjoint_identity_with_the_tangent_linear_step(n, tag, B, forcing, step_counts, dev):
    """<J dw, g> = <dw, J^T g> in the real inner product, J dw from op.tangent_step, J^T g from op.adjoint_step: the smallest
    plan with a ragged batch (8), radix-5 / radix-3 first passes (80, 96), cross-lane rows (512), split plans with whole-column
    tiles in the adjoint sweep (1024), one-sample chunks (2048)."""
    w0, dw, g, _ = (x.to(dev) for x in V.inputs(n, tag, B))
    op = V.build_op(n, tag, forcing, dev)
    dt, tol = V.dt_of(n), _tol(tag, 1e-12, 1e-5)
    for steps in step_counts:
        w_t, jdw = op.tangent_step(w0, dw, dt, steps)
        w_new, jtg = op.adjoint_step(w0, g, dt, steps)
        lhs, rhs = ns2d_ops.real_inner(jdw, g).item(), ns2d_ops.real_inner(dw, jtg).item()
        scale = (torch.linalg.norm(jdw) * torch.linalg.norm(g)).item()
        e_w = rel_l2(w_new, w_t)
        print(f"n={n} {tag} steps={steps}: <Jdw,g> {lhs:.12e} <dw,JTg> {rhs:.12e} defect/scale {abs(lhs - rhs) / scale:.3e} "
              f"state vs tangent_step {e_w:.3e}")
        assert abs(lhs - rhs) <= tol * scale, steps
        assert e_w <= _tol(tag, 1e-12, 2e-5), steps


# ----------------------------------------------------------------------------- 3. against the per-stage node chain
@pytest.mark.parametrize("n,tag,B,steps,chunked", [(64, "f64", 3, 2, False), (256, "f32", 2, 2, False), (1024, "f64", 6, 1, True),
                                                   (512, "f64", 20, 1, True)])
def test_one_node_path_matches_the_per_stage_nodes(n, tag, B, steps, chunked, dev, monkeypatch):
    """wbar of FusedSteps against TCFD_FUSED_ADJOINT=0 for a loss of BOTH outputs (w_new, dwdt), and adjoint_step's folding of
    g_dwdt against the same; 1024 x 6 and 512 x 20 run in several chunks per call."""
    w0, _, g, g2 = (x.to(dev) for x in V.inputs(n, tag, B))
    op = V.build_op(n, tag, "kolmogorov", dev)
    dt, tol = V.dt_of(n), _tol(tag, 1e-10, 2e-5)
    if chunked:
        per = V.fields_per_chunk(op, w0, B)
        assert 0 < per < B, f"the case is meant to run in several chunks, got {per} of {B} fields per chunk"
    g2 = g2 * (steps * dt)          # the cotangent of dwdt = (w_new - w) / (steps dt), scaled to weigh like g
    grads = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("TCFD_FUSED_ADJOINT", flag)
        grads[flag], node = V.grad_through_forward(op, w0, dt, steps, g, g2)
        assert ("FusedSteps" in node) == (flag == "1"), (node, flag)
    monkeypatch.delenv("TCFD_FUSED_ADJOINT")
    e_nodes = rel_l2(grads["1"], grads["0"])
    _, wbar = op.adjoint_step(w0, g, dt, steps, g_dwdt=g2)
    e_fold = rel_l2(wbar, grads["0"])
    only_state = rel_l2(op.adjoint_step(w0, g, dt, steps)[1], grads["0"])
    print(f"n={n} {tag} B={B} steps={steps}: FusedSteps vs per-stage {e_nodes:.3e}, adjoint_step with g_dwdt {e_fold:.3e} "
          f"(without g_dwdt it would be {only_state:.3e})")
    assert e_nodes <= tol and e_fold <= tol
    assert only_state > 100 * tol, "the dwdt term of the loss is too small to check its folding"


# ----------------------------------------------------------------------------- 4. exact properties, bitwise
@pytest.mark.parametrize("n,tag,B,solver", [(16, "f64", 3, "rk4"), (64, "f32", 3, "rk4"), (64, "f64", 3, "imex2"), (96, "f64", 2, "rk4")])
def test_reproducible_and_batch_independent_bitwise(n, tag, B, solver, dev):
    op = V.build_op(n, tag, "kolmogorov", dev, solver=solver)
    w0, _, g, _ = (x.to(dev) for x in V.inputs(n, tag, B))
    dt = V.dt_of(n)
    w1, b1 = op.adjoint_step(w0, g, dt, 3)
    w2, b2 = op.adjoint_step(w0, g, dt, 3)
    assert torch.equal(w1, w2) and torch.equal(b1, b2)
    # linear in the cotangent: zero gives zero, a power of two scales every intermediate exactly
    assert (op.adjoint_step(w0, torch.zeros_like(g), dt, 3)[1] == 0).all()
    assert torch.equal(op.adjoint_step(w0, 2 * g, dt, 3)[1], 2 * b1)
    # K steps in one call equal K one-step calls chained backwards
    states = [w0]
    for _ in range(2):
        states.append(op.adjoint_step(states[-1], g, dt, 1)[0])
    bar = g
    for s in reversed(states):
        bar = op.adjoint_step(s, bar, dt, 1)[1]
    assert torch.equal(bar, b1)
    for b in range(B):
        wa, ba = op.adjoint_step(w0[b:b + 1], g[b:b + 1], dt, 3)
        assert torch.equal(wa[0], w1[b]) and torch.equal(ba[0], b1[b]), b


@pytest.mark.parametrize("n,B,alone", [(1024, 6, (0, 2, 3, 5)), (512, 20, (0, 9, 10, 19))])
def test_several_chunks_per_call_equal_the_samples_alone(n, B, alone, dev):
    """fp64 batches the library cuts into several chunks: the samples on both sides of a chunk boundary carry the bits of their
    run alone, and a second run gives the same bits."""
    op = V.build_op(n, "f64", "kolmogorov", dev)
    w0, _, g, _ = (x.to(dev) for x in V.inputs(n, "f64", B))
    per = V.fields_per_chunk(op, w0, B)
    assert 0 < per < B, "the case is meant to run in several chunks"
    assert alone[0] // per != alone[-1] // per, (per, alone)
    dt = V.dt_of(n)
    w1, b1 = op.adjoint_step(w0, g, dt, 2)
    w2, b2 = op.adjoint_step(w0, g, dt, 2)
    assert torch.equal(w1, w2) and torch.equal(b1, b2)
    for b in alone:
        wa, ba = op.adjoint_step(w0[b:b + 1], g[b:b + 1], dt, 2)
        assert torch.equal(wa[0], w1[b]) and torch.equal(ba[0], b1[b]), b


@pytest.mark.parametrize("n,tag,solver", [(64, "f64", "rk4"), (32, "f32", "imex2")])
def test_checkpointing_gives_the_same_bits(n, tag, solver, dev):
    """checkpoint_every = 2, 3 at steps = 7 (a short last segment either way): the refilled states come from the same calls on
    the same inputs, so the cotangent is bit-equal to the one from all seven saved inputs."""
    op = V.build_op(n, tag, "kolmogorov", dev, solver=solver)
    w0, _, g, g2 = (x.to(dev) for x in V.inputs(n, tag, 3))
    dt = V.dt_of(n)
    w1, b1 = op.adjoint_step(w0, g, dt, 7, g_dwdt=g2)
    for every in (2, 3, 7, 50):
        wc, bc = op.adjoint_step(w0, g, dt, 7, g_dwdt=g2, checkpoint_every=every)
        assert torch.equal(wc, w1) and torch.equal(bc, b1), every


def test_cotangent_in_place_gives_the_bits_of_the_separate_output(dev):
    """g_in aliasing g_out (the raw call through _HipPlan.step_vjp): RK4-CN and the order-2 schedule, two steps."""
    from torch_cfd_amd import autograd as ad

    for solver in ("rk4", "imex2"):
        op = V.build_op(64, "f64", "kolmogorov", dev, solver=solver)
        w0, _, g, _ = (x.to(dev) for x in V.inputs(64, "f64", 3))
        plan = op._plan(w0)
        sc = op._schedule(op.solver, op.solver.params, 1e-3)
        saved = torch.stack([w0, op(w0, 1e-3, 1)[0]]).contiguous()
        pre, post = ad.FusedExplicitTerms._tables(op, plan, dev)
        kw = dict(fa=sc["fa"], mu_den=sc["mu_den"], base0=sc["base0"])
        keep_saved, keep_g = saved.clone(), g.clone()
        apart = plan.step_vjp(saved, g, pre, post, sc["beta"], sc["gdt"], sc["mu"], **kw)
        assert torch.equal(saved, keep_saved) and torch.equal(g, keep_g)
        inplace = g.clone()
        assert plan.step_vjp(saved, inplace, pre, post, sc["beta"], sc["gdt"], sc["mu"], out=inplace, **kw) is inplace
        assert torch.equal(inplace, apart), solver
        assert torch.equal(apart, op.adjoint_step(w0, g, 1e-3, 2)[1]), solver


def test_input_shapes_and_the_empty_batch(dev):
    op = V.build_op(64, "f64", "kolmogorov", dev)
    w0, _, g, g2 = (x.to(dev) for x in V.inputs(64, "f64", 4))
    w, b = op.adjoint_step(w0, g, 1e-3, 2)
    w1, b1 = op.adjoint_step(w0[0], g[0], 1e-3, 2)
    assert w1.shape == (64, 33) and torch.equal(w1, w[0]) and torch.equal(b1, b[0])
    w4, b4 = op.adjoint_step(w0.reshape(2, 2, 64, 33), g.reshape(2, 2, 64, 33), 1e-3, 2)
    assert w4.shape == (2, 2, 64, 33) and torch.equal(w4.reshape(4, 64, 33), w) and torch.equal(b4.reshape(4, 64, 33), b)
    bd = op.adjoint_step(w0, g, 1e-3, 2, g_dwdt=g2)[1]
    bd4 = op.adjoint_step(w0.reshape(2, 2, 64, 33), g.reshape(2, 2, 64, 33), 1e-3, 2, g_dwdt=g2.reshape(2, 2, 64, 33))[1]
    assert torch.equal(bd4.reshape(4, 64, 33), bd) and torch.equal(op.adjoint_step(w0[0], g[0], 1e-3, 2, g_dwdt=g2[0])[1], bd[0])
    we, be = op.adjoint_step(w0[:0], g[:0], 1e-3, g_dwdt=g2[:0])
    assert we.shape == (0, 64, 33) and be.shape == (0, 64, 33)
    # the autograd route: the same shapes give the bits of the explicit call, and an empty batch that requires grad goes through
    for state, cot, want in ((w0[0], g[0], b1), (w0, g, b), (w0.reshape(2, 2, 64, 33), g.reshape(2, 2, 64, 33), b4)):
        wbar, node = V.grad_through_forward(op, state, 1e-3, 2, cot)
        assert "FusedSteps" in node and wbar.shape == state.shape and torch.equal(wbar, want)
    empty = w0[:0].clone().requires_grad_(True)
    out, _ = op(empty, 1e-3, 2)
    assert out.shape == (0, 64, 33)
    out.abs().sum().backward()
    assert empty.grad is not None and empty.grad.shape == (0, 64, 33)


def test_refusals(dev):
    """The library's TCFD_EINVAL cases (each names itself in tcfd_last_error), the short workspace, and the Python errors of
    adjoint_step; on the same configurations the autograd route keeps working on the paths it took before."""
    import torch_cfd_amd as tc
    from torch_cfd_amd import autograd as ad

    op = V.build_op(64, "f64", "kolmogorov", dev)
    w0, _, g, _ = (x.to(dev) for x in V.inputs(64, "f64", 2))
    plan = op._plan(w0)
    lib, h = plan.lib, plan.handle
    sc = op._schedule(op.solver, op.solver.params, 1e-3)
    beta, gdt, mu = (tc._lib.darray(sc[k]) for k in ("beta", "gdt", "mu"))
    nst = len(sc["beta"])
    pre, post = ad.FusedExplicitTerms._tables(op, plan, dev)
    saved = torch.stack([w0, w0]).contiguous()
    out = torch.full_like(g, 7.0)
    need = lib.tcfd_ns2d_step_vjp_workspace_bytes(h, 2, nst)
    assert need > 0 and lib.tcfd_ns2d_step_vjp_workspace_bytes(h, 0, nst) == 0
    assert lib.tcfd_ns2d_step_vjp_workspace_bytes(h, 2, 0) == 0 and lib.tcfd_ns2d_step_vjp_workspace_bytes(h, 2, 33) == 0
    assert lib.tcfd_ns2d_step_vjp_workspace_bytes(h, 2, 32) > need
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(saved_p=saved.data_ptr(), g_p=g.data_ptr(), pre_p=pre.data_ptr(), post_p=post.data_ptr(), out_p=out.data_ptr(),
             nstages=nst, steps=2, beta_p=beta, ws_bytes=need):
        with torch.cuda.device(dev):
            return lib.tcfd_ns2d_step_vjp(h, saved_p, g_p, pre_p, post_p, out_p, 2, nstages, None, beta_p, gdt, mu, None, None,
                                          steps, ws.data_ptr(), ws_bytes, None)

    for kw, word in (({"saved_p": None}, b"null"), ({"g_p": None}, b"null"), ({"pre_p": None}, b"null"), ({"post_p": None}, b"null"),
                     ({"out_p": None}, b"null"), ({"beta_p": None}, b"null"), ({"steps": 0}, b"steps"), ({"steps": -3}, b"steps"),
                     ({"nstages": 0}, b"nstages"), ({"nstages": 33}, b"nstages"),
                     ({"out_p": saved.data_ptr()}, b"saved"), ({"out_p": saved[1].data_ptr()}, b"saved"),
                     ({"out_p": g.data_ptr() + 16}, b"g_out"), ({"out_p": g[1].data_ptr()}, b"g_out")):
        assert call(**kw) == TCFD_EINVAL, kw
        assert word in lib.tcfd_last_error(), (kw, lib.tcfd_last_error())
    assert call(ws_bytes=need - 1) == TCFD_EWORKSPACE and b"workspace" in lib.tcfd_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call wrote its output"
    assert call() == 0
    # adjoint_step: a cotangent that requires grad, trainable coefficients, a foreign solver, a grid outside the fused sizes
    with pytest.raises(NotImplementedError, match="requires grad"):
        op.adjoint_step(w0, g.clone().requires_grad_(True), 1e-3)
    with pytest.raises(NotImplementedError, match="requires grad"):
        op.adjoint_step(w0.clone().requires_grad_(True), g, 1e-3)
    with pytest.raises(NotImplementedError, match="requires grad"):
        op.adjoint_step(w0, g, 1e-3, g_dwdt=g.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        op.adjoint_step(w0, g[:1], 1e-3)
    with pytest.raises(ValueError):
        op.adjoint_step(w0, g, 1e-3, steps=0)
    with pytest.raises(ValueError):
        op.adjoint_step(w0, g, 1e-3, checkpoint_every=0)
    trainable = V.build_op(64, "f64", "kolmogorov", dev, solver=tc.RK4CrankNicolsonStepper(requires_grad=True))
    with pytest.raises(NotImplementedError, match="trainable"):
        trainable.adjoint_step(w0, g, 1e-3)

    class Foreign:
        def __call__(self, u, dt, equation):
            return tc.run_stage_schedule(u, equation, op.solver.stage_schedule(op.solver.params, dt))

    foreign = V.build_op(64, "f64", "kolmogorov", dev, solver=Foreign())
    with pytest.raises(NotImplementedError, match="stepper of this module"):
        foreign.adjoint_step(w0, g, 1e-3)
    small = V.build_op(48, "f64", "none", dev)
    w48 = torch.fft.rfft2(torch.randn(2, 48, 48, dtype=torch.float64)).to(dev)
    with pytest.raises(NotImplementedError, match="fused grid sizes"):
        small.adjoint_step(w48, w48.clone(), 1e-3)
    # ... while forward() with a state that requires grad still differentiates on those configurations
    want = op.adjoint_step(w0, g, 1e-3)[1]
    for other, state, cot in ((trainable, w0, g), (foreign, w0, g), (small, w48, w48)):
        wbar, node = V.grad_through_forward(other, state, 1e-3, 1, cot)
        assert "FusedSteps" not in node and torch.isfinite(torch.view_as_real(wbar)).all()
        if other is not small:
            assert rel_l2(wbar, want) <= 1e-10


@pytest.mark.parametrize("forcing", ["none", "kolmogorov"])
def test_gradient_penalty_through_the_one_node_path(forcing, dev, monkeypatch):
    """create_graph=True through FusedSteps (it restates itself on the per-stage nodes, which restate themselves as tensor ops):
    d/dw |dL/dw|^2 at steps = 2 against the tensor-op path, the gradient penalty of tests/test_ns2d_gpu.py; with a forcing too,
    and with the per-stage nodes switched to their tensor-op form between the forward and the backward (the restatement must
    carry the forcing itself then: the penalty sees the stage states, which a dropped forcing would change)."""
    from oracle import ns2d as O

    n, B = 32, 2
    op = V.build_op(n, "f64", forcing, dev)
    w0 = torch.stack([torch.fft.rfft2(O.mcwilliams_vorticity(n, V.L, 4, 11 + s, torch.float64)) for s in range(B)]).to(dev)
    pen, first = {}, {}
    for flag in ("1", "0", "flipped"):
        monkeypatch.setenv("TCFD_FUSED_VJP", "0" if flag == "0" else "1")
        monkeypatch.setenv("TCFD_FUSED_STAGE", "0" if flag == "0" else "1")
        w = w0.clone().requires_grad_(True)
        out, dwdt = op(w, 2e-3, steps=2)
        assert ("FusedSteps" in V.node_name(out)) == (flag != "0")
        loss = out.abs().pow(4).sum() + dwdt.abs().pow(2).sum() * 1e-4
        if flag == "flipped":
            monkeypatch.setenv("TCFD_FUSED_VJP", "0")
        (gw,) = torch.autograd.grad(loss, w, create_graph=True)
        assert gw.requires_grad
        first[flag] = gw.detach()
        (gp,) = torch.autograd.grad(gw.abs().pow(2).sum(), w)
        pen[flag] = gp
    print(f"first derivative {rel_l2(first['1'], first['0']):.3e}, penalty gradient {rel_l2(pen['1'], pen['0']):.3e}")
    assert rel_l2(first["1"], first["0"]) <= 1e-10 and rel_l2(first["flipped"], first["0"]) <= 1e-10
    assert torch.linalg.norm(pen["0"]) > 0 and rel_l2(pen["1"], pen["0"]) <= 1e-9 and rel_l2(pen["flipped"], pen["0"]) <= 1e-9


# ----------------------------------------------------------------------------- 5. memory contract (guarded, poisoned buffers)
CONTRACT_PLANS = [(8, "f64", 5), (64, "f32", 3), (96, "f32", 2), (1024, "f64", 6), (2048, "f32", 2)]


@pytest.mark.parametrize("n, tag, batch", CONTRACT_PLANS, ids=[f"n{n}-{t}-b{b}" for n, t, b in CONTRACT_PLANS])
def test_memory_contract(n, tag, batch):
    """tcfd_ns2d_step_vjp through guard_ops.run_guarded, on the operators and with the ``guard`` protocol of
    tests/test_memory_contract_gpu.py: saved, g_out, pre and post come back unchanged, nothing is written outside g_in and the
    workspace, every element of g_in is written, the bits do not depend on the poison or on a dirty workspace and equal the
    wrapper's, the call works with exactly tcfd_ns2d_step_vjp_workspace_bytes and refuses one byte less without touching
    anything -- RK4-CN and the order-2 schedule (base0), two steps, and g_in aliasing g_out; chunked at 1024 x 6, one-sample
    chunks at 2048."""
    import test_memory_contract_gpu as M
    from torch_cfd_amd.autograd import FusedExplicitTerms

    s, lib = M.ns(n, tag, batch), M._L()
    B = s.batch
    assert lib.tcfd_ns2d_step_vjp_workspace_bytes(s.h, 0, 5) == 0
    if n >= 1024:    # chunked: the scratch stops growing at one chunk
        assert s.chunk(B) < B and lib.tcfd_ns2d_step_vjp_workspace_bytes(s.h, B, 5) < lib.tcfd_ns2d_step_vjp_workspace_bytes(s.h, 1, 5) * B
    pre, post = FusedExplicitTerms._tables(s.op, s.plan, M._dev())
    for sc in (s.op._schedule(s.op.solver, s.op.solver.params, s.dt), s.imex2.stage_schedule(s.imex2.params, s.dt)):
        beta, gdt, mu, nst = sc["beta"], sc["gdt"], sc["mu"], len(sc["beta"])
        ints = (ctypes.c_int * nst)(*[int(v) for v in sc["base0"]]) if sc["base0"] is not None else None
        need = lib.tcfd_ns2d_step_vjp_workspace_bytes(s.h, B, nst)
        assert need == (12 + nst) * lib.tcfd_ns2d_workspace_bytes(s.h, s.chunk(B)) // 8      # 12 + nstages chunk-sized fields
        kw = dict(fa=sc["fa"], mu_den=sc["mu_den"], base0=sc["base0"])
        saved = torch.stack([s.w, s.plan.step(s.w, beta, gdt, mu, 1, 1.0, False, **kw)[0]]).contiguous()
        ref = s.plan.step_vjp(saved, s.w2, pre, post, beta, gdt, mu, **kw)

        def call(P, gin, ws, nb):
            return lib.tcfd_ns2d_step_vjp(s.h, P("saved"), P("g"), P("pre"), P("post"), P(gin), B, nst, M._darr(sc["fa"]),
                                          M._darr(beta), M._darr(gdt), M._darr(mu), M._darr(sc["mu_den"]), ints, 2, ws, nb,
                                          M._stream())

        ins = {"saved": saved, "g": s.w2, "pre": pre, "post": post}
        M.guard(f"tcfd_ns2d_step_vjp nstages={nst}", ins, {"gin": s.out()}, lambda P, ws, nb: call(P, "gin", ws, nb), need,
                {"gin": ref})
        M.guard(f"tcfd_ns2d_step_vjp nstages={nst} in place", ins, {"g": s.out()}, lambda P, ws, nb: call(P, "g", ws, nb), need,
                {"g": ref})
    if n >= 1024:
        M.ns.cache_clear()     # the large plans and inputs do not outlive the case
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 6. memory
def test_backward_keeps_one_field_per_step(dev, monkeypatch):
    """256^2 x 8 complex128, RK4-CN, 8 steps: the peak of loss + backward through FusedSteps over the baseline is at most
    (steps + 4) batch-sized fields (the saved inputs, the result, its cotangent, the gradient, one temporary of the loss) plus
    the two workspaces the library reports, and below the per-stage chain's, which keeps nstages x steps fields."""
    n, B, steps, dt = 256, 8, 8, 1e-3
    op = V.build_op(n, "f64", "kolmogorov", dev)
    w0, _, g, _ = (x.to(dev) for x in V.inputs(n, "f64", B))
    field = w0.numel() * w0.element_size()
    plan = op._plan(w0)
    nst = len(op._schedule(op.solver, op.solver.params, dt)["beta"])
    ws_bytes = plan.lib.tcfd_ns2d_workspace_bytes(plan.handle, B) + plan.lib.tcfd_ns2d_step_vjp_workspace_bytes(plan.handle, B, nst)
    gr = torch.view_as_real(g)

    def run(flag, w_in, cot):
        monkeypatch.setenv("TCFD_FUSED_ADJOINT", flag)
        w = w_in.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out, _ = op(w, dt, steps)
        (torch.view_as_real(out) * cot).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - base, w.grad

    for flag in ("1", "0"):          # the (plane-sized) tables of both paths exist before anything is measured
        run(flag, w0[:1], gr[:1])
    peak_fused, grad_fused = run("1", w0, gr)
    peak_nodes, grad_nodes = run("0", w0, gr)
    print(f"peak over baseline: FusedSteps {peak_fused / field:.2f} fields ({(peak_fused - ws_bytes) / field:.2f} without the "
          f"reported workspaces), per-stage nodes {peak_nodes / field:.2f} fields (nstages x steps = {nst * steps}); "
          f"one field = {field} bytes")
    assert rel_l2(grad_fused, grad_nodes) <= 1e-10
    assert peak_fused <= (steps + 4) * field + ws_bytes
    assert peak_fused < peak_nodes
