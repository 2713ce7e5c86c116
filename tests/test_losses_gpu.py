"""On the device: ResidualLoss, LpLoss, L2Loss2d and BochnerNorm (torch_cfd_amd.losses on csrc/tcfd_residual.hip) against the
reference's stored outputs (tests/golden/losses.npz) and against the plain-torch restatement tests/losses_ops.py in float64 on the
same device.  Bars: float64 value 1e-11, gradient 1e-10 (relative L2); float32 2e-6 and 2e-5 -- the project's bars for loss and
gradient parity (tests/test_fno_gpu.py); the reference's own float32 deviation is 2e-8 .. 3e-7 on these inputs."""
import os

import numpy as np
import pytest
import torch

import losses_ops as ops
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "losses.npz"))
VAL64, GRAD64, VAL32, GRAD32 = 1e-11, 1e-10, 2e-6, 2e-5
DEV = "cuda"


def gold(name):
    return torch.from_numpy(np.asarray(GOLD[name]))


def check(what, got, want, bar):
    err = ops.relerr(got.detach().cpu(), want.detach().cpu())
    print(f"{what}: {err:.3e} (bar {bar:.0e})")
    assert err <= bar, (what, err, bar)


def make(b, n, nt, norm="ortho", dtype=torch.float64):
    from torch_cfd_amd.losses import ResidualLoss

    torch.set_default_dtype(dtype)
    try:
        return ResidualLoss(batch_size=b, visc=ops.residual_visc(n), n_grid=n, n_t=nt, delta_t=ops.RESIDUAL_DELTA_T, norm=norm)
    finally:
        torch.set_default_dtype(torch.float32)


def inputs(b, n, nt, dtype=torch.float64):
    return tuple(z.to(DEV) for z in ops.residual_inputs(b, n, nt, dtype))


def ops_loss(w, psi=None, f=None, norm="ortho", table_dtype=None):
    n = w.shape[1]
    return ops.residual_loss(w, psi, f, visc=ops.residual_visc(n), delta_t=ops.RESIDUAL_DELTA_T, norm=norm, table_dtype=table_dtype)


def value_and_grads(fn, w, f=None, psi=None):
    leaves = [z.detach().clone().requires_grad_(True) if z is not None else None for z in (w, f, psi)]
    loss = fn(*leaves)
    gs = torch.autograd.grad(loss, [z for z in leaves if z is not None])
    return loss.detach(), gs


@pytest.mark.parametrize("shape", ops.RESIDUAL_SHAPES)
def test_residual_matches_golden(shape):
    b, n, nt = shape
    w, f, psi = inputs(b, n, nt)
    tag = f"res_{b}_{n}_{nt}"
    for norm in ("ortho", "backward", "forward"):
        m = make(b, n, nt, norm)
        with torch.no_grad():
            check(f"{tag} {norm} f", m(w, f=f), gold(f"{tag}_{norm}_f"), VAL64)
            check(f"{tag} {norm} no f", m(w), gold(f"{tag}_{norm}_nof"), VAL64)
            check(f"{tag} {norm} psi", m(w, psi=psi, f=f), gold(f"{tag}_{norm}_psi"), VAL64)
    m = make(b, n, nt)
    if n <= 32:
        val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
        check(f"{tag} value under autograd", val, gold(f"{tag}_ortho_f"), VAL64)
        check(f"{tag} grad w", gw, gold(f"{tag}_gw"), GRAD64)
        if n == 16:
            check(f"{tag} grad f", gf, gold(f"{tag}_gf"), GRAD64)
    if (n, nt) == (16, 5):
        _, (gw,) = value_and_grads(lambda a, *_: m(a), w)
        check(f"{tag} grad w without f", gw, gold(f"{tag}_nof_gw"), GRAD64)
        _, (gw, gf, gp) = value_and_grads(lambda a, c, p: m(a, psi=p, f=c), w, f, psi)
        check(f"{tag} grad w with psi", gw, gold(f"{tag}_psi_gw"), GRAD64)
        check(f"{tag} grad psi", gp, gold(f"{tag}_psi_gpsi"), GRAD64)


@pytest.mark.parametrize("shape", ops.RESIDUAL_SHAPES)
def test_residual_float32_matches_golden(shape):
    b, n, nt = shape
    w, f, _ = inputs(b, n, nt, torch.float32)
    tag = f"res_{b}_{n}_{nt}"
    m = make(b, n, nt, dtype=torch.float32)
    val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
    assert val.dtype == torch.float32 and gw.dtype == torch.float32
    print(f"{tag}: the reference's own float32 deviation {float(GOLD[tag + '_f32_dev']):.2e}")
    check(f"{tag} float32 value", val, gold(f"{tag}_ortho_f"), VAL32)
    if n <= 32:
        check(f"{tag} float32 grad w", gw, gold(f"{tag}_gw"), GRAD32)
    if n == 16:
        check(f"{tag} float32 grad f", gf, gold(f"{tag}_gf"), GRAD32)


CORNERS = ((2, 16, 5), (3, 16, 10), (2, 32, 7), (2, 16, 1), (2, 64, 12), (1, 64, 40), (2, 80, 6), (2, 96, 4))


@pytest.mark.parametrize("shape", CORNERS)
def test_residual_corners_against_ops(shape):
    b, n, nt = shape
    w, f, _ = inputs(b, n, nt)
    m = make(b, n, nt)
    val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
    ref, (rw, rf) = value_and_grads(lambda a, c, _: ops_loss(a, f=c), w, f)
    check(f"{shape} value", val, ref, VAL64)
    check(f"{shape} grad w", gw, rw, GRAD64)
    check(f"{shape} grad f", gf, rf, GRAD64)
    # only f needs a gradient: the backward pass stops after its row kernel
    fr = f.clone().requires_grad_(True)
    (gf2,) = torch.autograd.grad(m(w, f=fr), fr)
    assert torch.equal(gf2, gf)


def test_residual_sfno_output_size_float32():
    b, n, nt = 2, 256, 10
    w, f, _ = inputs(b, n, nt, torch.float32)
    m = make(b, n, nt, dtype=torch.float32)
    val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
    ref, (rw, rf) = value_and_grads(lambda a, c, _: ops_loss(a, f=c), w.double(), f.double())
    check("(2, 256, 10) float32 value", val, ref, VAL32)
    check("(2, 256, 10) float32 grad w", gw, rw, GRAD32)
    check("(2, 256, 10) float32 grad f", gf, rf, GRAD32)


@pytest.mark.parametrize("shape", ((3, 16, 10), (2, 80, 6)))
def test_residual_fused_against_composed(shape, monkeypatch):
    import torch_cfd_amd.losses as L

    b, n, nt = shape
    w, f, _ = inputs(b, n, nt)
    m = make(b, n, nt)
    calls = []
    orig = L.ResidualLoss._composed
    monkeypatch.setattr(L.ResidualLoss, "_composed", lambda self, *a: (calls.append(1), orig(self, *a))[1])
    val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
    assert not calls                                  # inside the cover nothing goes through the composed path
    monkeypatch.setenv("TCFD_RESIDUAL_FUSED", "0")
    cval, (cw, cf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
    assert calls
    check(f"{shape} fused vs composed value", val, cval, VAL64)
    check(f"{shape} fused vs composed grad w", gw, cw, GRAD64)
    check(f"{shape} fused vs composed grad f", gf, cf, GRAD64)


def test_residual_outside_cover_takes_composed_path(monkeypatch):
    import torch_cfd_amd.losses as L

    b, n, nt = 1, 16, 130                      # more time steps than the fused time transform holds
    w, f, _ = inputs(b, n, nt)
    m = make(b, n, nt)
    calls = []
    orig = L.ResidualLoss._composed
    monkeypatch.setattr(L.ResidualLoss, "_composed", lambda self, *a: (calls.append(1), orig(self, *a))[1])
    val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), w, f)
    assert calls
    ref, (rw, rf) = value_and_grads(lambda a, c, _: ops_loss(a, f=c), w, f)
    check("outside the cover: value", val, ref, VAL64)
    check("outside the cover: grad w", gw, rw, GRAD64)
    check("outside the cover: grad f", gf, rf, GRAD64)


def test_residual_float32_module_on_float64_data():
    b, n, nt = 2, 16, 5
    w, f, _ = inputs(b, n, nt)
    m = make(b, n, nt, dtype=torch.float32)
    assert m.lap.dtype == torch.float32
    with torch.no_grad():
        val = m(w, f=f)
    assert val.dtype == torch.float64
    check("float32-built module on float64 data", val, gold("res_2_16_5_mixed"), VAL64)
    _, (gw,) = value_and_grads(lambda a, *_: m(a, f=f), w)
    _, (rw,) = value_and_grads(lambda a, *_: ops_loss(a, f=f, table_dtype=torch.float32), w)
    check("float32-built module on float64 data: grad w", gw, rw, GRAD64)


def test_residual_zero_input_and_determinism():
    b, n, nt = 2, 16, 5
    m = make(b, n, nt)
    z = torch.zeros(b, n, n, nt, dtype=torch.float64, device=DEV)
    val, (gw, gf) = value_and_grads(lambda a, c, _: m(a, f=c), z, z)
    assert float(val) == 0.0
    assert torch.isfinite(gw).all() and torch.isfinite(gf).all() and not gw.any() and not gf.any()
    w, f, _ = inputs(b, n, nt)
    a = value_and_grads(lambda x, c, _: m(x, f=c), w, f)
    c = value_and_grads(lambda x, c, _: m(x, f=c), w, f)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1][0], c[1][0]) and torch.equal(a[1][1], c[1][1])


def test_residual_hessian_vector_product():
    b, n, nt = 2, 16, 5
    w, f, _ = inputs(b, n, nt)
    m = make(b, n, nt)
    v = torch.randn(w.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(DEV)

    def hvp(fn):
        wr = w.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(fn(wr), wr, create_graph=True)
        (hv,) = torch.autograd.grad((g * v).sum(), wr)
        return hv

    check("Hessian-vector product", hvp(lambda a: m(a, f=f)), hvp(lambda a: ops_loss(a, f=f)), 1e-8)


def test_residual_graph_capture():
    b, n, nt = 2, 32, 7
    w, f, _ = inputs(b, n, nt)
    m = make(b, n, nt)
    ws = w.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                  # plans, tables and kernel attributes are set up outside the capture
            (eager_g,) = torch.autograd.grad(m(ws, f=f), ws)
        eager = m(ws, f=f).detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = m(ws, f=f)
        (gw,) = torch.autograd.grad(loss, ws)
    loss.detach().zero_()
    gw.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), eager) and torch.equal(gw, eager_g)


# ---------------------------------------------------------------------------------------------- the small losses
def small_check(name, fn_mod, fn_ops, leaf, gold_val, gold_grad, dtype):
    vbar, gbar = (VAL64, GRAD64) if dtype == torch.float64 else (VAL32, GRAD32)
    x = leaf.to(DEV, dtype).requires_grad_(True)
    val = fn_mod(x)
    (g,) = torch.autograd.grad(val.sum(), x)
    x64 = leaf.to(DEV).requires_grad_(True)
    ref = fn_ops(x64)
    (rg,) = torch.autograd.grad(ref.sum(), x64)
    if gold_val is not None:
        check(f"{name} {dtype} value vs golden", val, gold_val, vbar)
    check(f"{name} {dtype} value vs ops", val, ref, vbar)
    check(f"{name} {dtype} grad vs ops", g, rg, gbar)
    if gold_grad is not None:
        check(f"{name} {dtype} grad vs golden", g, gold_grad, gbar)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_lp_loss(dtype):
    from torch_cfd_amd.losses import LpLoss

    x, y = ops.small_inputs(ops.SMALL_SHAPE_CH, 7)
    for name, kw in ops.LP_CASES.items():
        m = LpLoss(**kw)
        small_check(f"LpLoss {name}", lambda a: m(a, y.to(DEV, dtype)), lambda a: ops.lp_loss(a, y.to(DEV), **kw), x,
                    gold(f"lp_{name}"), gold(f"lp_{name}_gx") if name in ops.LP_GRAD_CASES else None, dtype)
    # a per-sample length (578) that is no multiple of the workgroup, and a gradient with respect to the target
    x17, y17 = ops.small_inputs((3, 2, 17, 17), 8)
    small_check("LpLoss odd p3 rel", lambda a: LpLoss(p=3, relative=True)(a, y17.to(DEV, dtype)),
                lambda a: ops.lp_loss(a, y17.to(DEV), p=3, relative=True), x17, gold("lp_odd_p3_rel"), None, dtype)
    small_check("LpLoss odd p2 abs", lambda a: LpLoss(p=2)(a, y17.to(DEV, dtype)), lambda a: ops.lp_loss(a, y17.to(DEV), p=2), x17,
                gold("lp_odd_p2_abs"), None, dtype)
    small_check("LpLoss grad y", lambda a: LpLoss(p=3, relative=True)(x17.to(DEV, dtype), a),
                lambda a: ops.lp_loss(x17.to(DEV), a, p=3, relative=True), y17, gold("lp_odd_p3_rel"), None, dtype)
    # several stage-one workgroups per sample
    xb, yb = ops.small_inputs((2, 3, 100, 101), 21)
    small_check("LpLoss two blocks", lambda a: LpLoss(p=2, relative=True)(a, yb.to(DEV, dtype)),
                lambda a: ops.lp_loss(a, yb.to(DEV), p=2, relative=True), xb, None, None, dtype)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_l2_loss_2d(dtype):
    from torch_cfd_amd.losses import L2Loss2d

    for name, kw in ops.L2_CASES.items():
        preds, targets, tg, K = ops.l2_case_inputs(kw["kmode"])
        m = L2Loss2d(metric_reduction=kw["metric_reduction"], weighted=kw["weighted"])
        cast = lambda z, dt: z.to(DEV, dt) if torch.is_tensor(z) else z
        tgs = tg if kw["with_grad"] else None
        small_check(f"L2Loss2d {name}", lambda a: m(a, cast(targets, dtype), cast(tgs, dtype), cast(K, dtype)),
                    lambda a: ops.l2_loss_2d(a, cast(targets, torch.float64), cast(tgs, torch.float64), cast(K, torch.float64),
                                             metric_reduction=kw["metric_reduction"], weighted=kw["weighted"]),
                    preds, gold(f"l2_{name}"), gold(f"l2_{name}_gp") if name in ops.L2_GRAD_CASES else None, dtype)
    # a mesh that is no multiple of anything, rectangular, more than one stencil workgroup per sample
    preds, targets = ops.small_inputs((2, 3, 67, 45), 31)
    (tg,) = ops.small_inputs((2, 6, 67, 45), 32, 1)
    m = L2Loss2d(metric_reduction="L2")
    small_check("L2Loss2d odd mesh", lambda a: m(a, targets.to(DEV, dtype), tg.to(DEV, dtype), 0.7),
                lambda a: ops.l2_loss_2d(a, targets.to(DEV), tg.to(DEV), torch.tensor(0.7, dtype=torch.float64), metric_reduction="L2"),
                preds, None, None, dtype)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_bochner_norm(dtype):
    from torch_cfd_amd.losses import BochnerNorm

    (u,) = ops.small_inputs(ops.SMALL_SHAPE_TL, 9, 1)
    n = ops.SMALL_SHAPE_TL[1]
    for name, kw in ops.BOCHNER_CASES.items():
        m = BochnerNorm(n_grid=n, **kw)
        leaf = u if kw["time_last"] else u.permute(0, 3, 1, 2).contiguous()
        small_check(f"BochnerNorm {name}", m, lambda a: ops.bochner_norm(a, n, **kw), leaf, gold(f"bochner_{name}"),
                    gold(f"bochner_{name}_gu") if name in ops.BOCHNER_GRAD_CASES else None, dtype)
    # sizes off every tile: 7 time steps (256 is no multiple of 7), a 19 x 19 mesh
    (v,) = ops.small_inputs((2, 19, 19, 7), 41, 1)
    m = BochnerNorm(n_grid=19, p=3, time_average=True, time_last=True)
    small_check("BochnerNorm odd", m, lambda a: ops.bochner_norm(a, 19, p=3, time_average=True, time_last=True), v, None, None, dtype)
