"""CPU-only checks of the losses added beside SobolevLoss (LpLoss, L2Loss2d, BochnerNorm, ResidualLoss): the plain-torch
restatement tests/losses_ops.py against the reference's stored outputs (tests/golden/losses.npz, written by
tests/golden/make_golden_losses.py), the sensitivity of the residual inputs to each term of the equation, and everything of the
classes that needs no device -- tables, attributes, argument checks."""
import os

import numpy as np
import pytest
import torch

import losses_ops as ops
from conftest import ROOT

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "losses.npz"))
TOL = 1e-12


def gold(name):
    return torch.from_numpy(np.asarray(GOLD[name]))


def rel(a, b):
    return ops.relerr(a, b)


@pytest.fixture(autouse=True)
def _float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize("shape", ops.RESIDUAL_SHAPES)
def test_residual_ops_match_golden(shape):
    b, n, nt = shape
    w, f, psi = ops.residual_inputs(b, n, nt)
    kw = dict(visc=ops.residual_visc(n), delta_t=ops.RESIDUAL_DELTA_T)
    tag = f"res_{b}_{n}_{nt}"
    for norm in ("ortho", "backward", "forward"):
        assert rel(ops.residual_loss(w, f=f, norm=norm, **kw), gold(f"{tag}_{norm}_f")) <= TOL
        assert rel(ops.residual_loss(w, norm=norm, **kw), gold(f"{tag}_{norm}_nof")) <= TOL
        assert rel(ops.residual_loss(w, psi=psi, f=f, norm=norm, **kw), gold(f"{tag}_{norm}_psi")) <= TOL
    if n <= 32:
        wr, fr, pr = (z.clone().requires_grad_(True) for z in (w, f, psi))
        gw, gf = torch.autograd.grad(ops.residual_loss(wr, f=fr, **kw), (wr, fr))
        assert rel(gw, gold(f"{tag}_gw")) <= TOL
        if n == 16:
            assert rel(gf, gold(f"{tag}_gf")) <= TOL
        if (n, nt) == (16, 5):
            (g,) = torch.autograd.grad(ops.residual_loss(wr, **kw), wr)
            assert rel(g, gold(f"{tag}_nof_gw")) <= TOL
            gw, gp = torch.autograd.grad(ops.residual_loss(wr, psi=pr, f=fr, **kw), (wr, pr))
            assert rel(gw, gold(f"{tag}_psi_gw")) <= TOL and rel(gp, gold(f"{tag}_psi_gpsi")) <= TOL


def test_residual_ops_float32_tables_on_float64_data():
    b, n, nt = 2, 16, 5
    w, f, _ = ops.residual_inputs(b, n, nt)
    v = ops.residual_loss(w, f=f, visc=ops.residual_visc(n), delta_t=ops.RESIDUAL_DELTA_T, table_dtype=torch.float32)
    assert v.dtype == torch.float64 and rel(v, gold("res_2_16_5_mixed")) <= TOL
    # the rounding of the tables is visible: far from the all-float64 value on the scale of TOL
    assert rel(v, gold("res_2_16_5_ortho_f")) > 1e-10


@pytest.mark.parametrize("shape", ops.RESIDUAL_SHAPES)
def test_sensitivity(shape):
    """Dropping any one term of the equation moves the value by at least 1e-3: a broken term cannot hide behind the others.
    No row norm comes near zero either (the gradient of the norm is smooth at these inputs)."""
    b, n, nt = shape
    w, f, _ = ops.residual_inputs(b, n, nt)
    kw = dict(visc=ops.residual_visc(n), delta_t=ops.RESIDUAL_DELTA_T)
    full = float(ops.residual_loss(w, f=f, **kw))
    for term in ("time", "convection", "viscous", "forcing"):
        dropped = float(ops.residual_loss(w, f=f, drop=term, **kw))
        assert abs(dropped - full) / abs(full) >= 1e-3, (term, dropped, full)


def test_small_ops_match_golden():
    x, y = ops.small_inputs(ops.SMALL_SHAPE_CH, 7)
    for name, kw in ops.LP_CASES.items():
        xr = x.clone().requires_grad_(True)
        val = ops.lp_loss(xr, y, **kw)
        assert rel(val, gold(f"lp_{name}")) <= TOL, name
        if name in ops.LP_GRAD_CASES:
            (g,) = torch.autograd.grad(val.sum(), xr)
            assert rel(g, gold(f"lp_{name}_gx")) <= TOL, name
    x17, y17 = ops.small_inputs((3, 2, 17, 17), 8)
    assert rel(ops.lp_loss(x17, y17, p=3, relative=True), gold("lp_odd_p3_rel")) <= TOL
    assert rel(ops.lp_loss(x17, y17, p=2), gold("lp_odd_p2_abs")) <= TOL
    for name, kw in ops.L2_CASES.items():
        preds, targets, tg, K = ops.l2_case_inputs(kw["kmode"])
        pr = preds.clone().requires_grad_(True)
        val = ops.l2_loss_2d(pr, targets, tg if kw["with_grad"] else None, K, metric_reduction=kw["metric_reduction"],
                             weighted=kw["weighted"])
        assert rel(val, gold(f"l2_{name}")) <= TOL, name
        if name in ops.L2_GRAD_CASES:
            (g,) = torch.autograd.grad(val, pr)
            assert rel(g, gold(f"l2_{name}_gp")) <= TOL, name
    (u,) = ops.small_inputs(ops.SMALL_SHAPE_TL, 9, 1)
    for name, kw in ops.BOCHNER_CASES.items():
        ur = (u if kw["time_last"] else u.permute(0, 3, 1, 2).contiguous()).clone().requires_grad_(True)
        val = ops.bochner_norm(ur, ops.SMALL_SHAPE_TL[1], **kw)
        assert rel(val, gold(f"bochner_{name}")) <= TOL, name
        if name in ops.BOCHNER_GRAD_CASES:
            (g,) = torch.autograd.grad(val, ur)
            assert rel(g, gold(f"bochner_{name}_gu")) <= TOL, name


def test_central_diff_matches_golden():
    from torch_cfd_amd.losses import central_diff

    (x, _) = ops.small_inputs(ops.SMALL_SHAPE_CH, 7)
    gx, gy = central_diff(x)
    assert torch.equal(gx, gold("cd_gx")) and torch.equal(gy, gold("cd_gy"))
    ox, oy = ops.central_diff(x)
    assert torch.equal(ox, gx) and torch.equal(oy, gy)
    # channel-last input: the same differences, channels moved
    xl = x.permute(0, 2, 3, 1)
    cx, cy = central_diff(xl, channel_last=True)
    ex, ey = ops.central_diff(xl.transpose(-1, -3))
    assert torch.equal(cx, ex.transpose(-3, -1)) and torch.equal(cy, ey.transpose(-3, -1))
    hx, _ = central_diff(x, h=0.5)
    assert torch.allclose(hx * 0.5, gx / 16)


def test_residual_tables_and_attributes():
    from torch_cfd_amd.losses import ResidualLoss

    m = ResidualLoss(batch_size=2, visc=ops.residual_visc(16), n_grid=16, n_t=5, delta_t=ops.RESIDUAL_DELTA_T)
    for name in ("kx", "ky", "kt", "lap"):
        t = getattr(m, name)
        assert tuple(t.shape) == (2, 16, 16, 5) and t.dtype == torch.float64
        assert torch.equal(t[0], gold(f"res_2_16_5_{name}")) and torch.equal(t[1], t[0]), name
    assert torch.all(m.lap[:, 0, 0, :] == 1)                      # the patched line, every kt
    assert float(m.kx[0, 8, 0, 0]) == -8.0                        # integer wavenumbers, Nyquist negative
    assert (m.batch_size, m.alpha, m.n_grid, m.n_t, m.delta_t, m.norm) == (2, 1e-1, 16, 5, ops.RESIDUAL_DELTA_T, "ortho")
    assert not list(m.buffers()) and not m.state_dict()           # plain attributes, not buffers
    d = ResidualLoss()
    assert (d.batch_size, d.alpha, d.visc, d.n_grid, d.n_t, d.delta_t, d.norm) == (1, 1e-1, 1e-3, 64, 40, 1e-2, "ortho")
    torch.set_default_dtype(torch.float32)
    m32 = ResidualLoss(batch_size=2, visc=ops.residual_visc(16), n_grid=16, n_t=5, delta_t=ops.RESIDUAL_DELTA_T)
    torch.set_default_dtype(torch.float64)
    assert m32.lap.dtype == torch.float32
    assert torch.equal(m32.lap[0], gold("res_2_16_5_lap_f32")) and torch.equal(m32.kt[0], gold("res_2_16_5_kt_f32"))
    # the tables of the restatement are the reference's too
    for got, name in zip(ops.residual_tables(16, 5, ops.RESIDUAL_DELTA_T), ("kx", "ky", "kt", "lap")):
        assert torch.equal(got, gold(f"res_2_16_5_{name}"))
    with pytest.raises(ValueError):
        ResidualLoss(norm="bogus")


def test_residual_argument_checks():
    from torch_cfd_amd.losses import ResidualLoss

    m = ResidualLoss(batch_size=2, n_grid=16, n_t=5)
    with pytest.raises(ValueError, match="batch"):
        m(torch.zeros(3, 16, 16, 5))
    with pytest.raises(ValueError, match="time steps"):
        m(torch.zeros(2, 16, 16, 6))
    with pytest.raises(ValueError, match="grid"):
        m(torch.zeros(2, 32, 32, 5))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 16, 16, 5), f=torch.zeros(2, 16, 16, 4))
    # batch_size 1 broadcasts to any batch: the check passes and the call stops at the device requirement (no CPU path)
    import torch_cfd_amd as tc

    with pytest.raises(tc._lib.TcfdError):
        ResidualLoss(batch_size=1, n_grid=16, n_t=5)(torch.zeros(3, 16, 16, 5))


def test_small_classes_construct():
    from torch_cfd_amd.losses import BochnerNorm, L2Loss2d, LpLoss, SobolevLoss

    bn = BochnerNorm(n_grid=16, dt=0.1, p=1, time_last=True)
    assert isinstance(bn, SobolevLoss) and (bn.n_grid, bn.dt, bn.p, bn.time_last) == (16, 0.1, 1, True)
    assert bn.mesh_weighted and bn.reduction and not bn.time_average and bn.relative
    d = BochnerNorm()
    assert (d.n_grid, d.dt, d.p, d.time_last, d.time_average) == (256, None, 2, False, False)
    with pytest.raises(ValueError, match="time_average"):
        d(torch.zeros(1, 2, 256, 256))                 # neither time_average nor dt
    lp = LpLoss()
    assert (lp.d, lp.p, lp.h, lp.size_average, lp.reduction, lp.relative) == (2, 2, None, True, True, False)
    with pytest.raises(AssertionError):
        LpLoss(p=0)
    l2 = L2Loss2d()
    assert (l2.h, l2.beta, l2.gamma, l2.metric_reduction, l2.noise, l2.eps) == (1 / 512, 1.0, 1e-1, "L1", 0.0, 1e-3)
    assert not (l2.regularizer or l2.weighted or l2.channel_last or l2.debug)
