"""The four losses of torch_cfd_amd.losses besides SobolevLoss as plain torch operations (torch.fft allowed: this is test code, the
yardstick of tests/test_losses_host.py and tests/test_losses_gpu.py, like tests/fvm_ops.py).  Written from the description of the
arithmetic, checked against tests/golden/losses.npz (the reference's own outputs) on the CPU."""
import math

import torch

RESIDUAL_SHAPES = ((2, 16, 5), (3, 16, 10), (2, 32, 7), (2, 64, 12), (2, 80, 6))     # (b, n, T): the golden cases
RESIDUAL_DELTA_T = 0.15


def residual_visc(n):
    return 8.0 / n**2


def residual_inputs(b, n, nt, dtype=torch.float64):
    """w, f, psi of one residual case: seeded CPU draws in float64 (cast afterwards), amplitudes at which every term of the
    equation moves the loss by more than 1e-3 (see ``test_sensitivity``)."""
    g = torch.Generator().manual_seed(3)
    w = 40 * torch.randn(b, n, n, nt, generator=g, dtype=torch.float64)
    f = 300 * torch.randn(b, n, n, nt, generator=g, dtype=torch.float64)
    psi = 0.05 * torch.randn(b, n, n, nt, generator=g, dtype=torch.float64)
    return w.to(dtype), f.to(dtype), psi.to(dtype)


def small_inputs(shape, seed, count=2, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype) for _ in range(count)]


def residual_tables(n, nt, delta_t, dtype=torch.float64):
    """kx, ky, kt, lap of shape (n, n, nt) in ``dtype``: integer wavenumbers (domain length 1), kt = fftfreq(nt, delta_t),
    lap = -4 pi^2 |k|^2 with the whole line lap[0, 0, :] set to 1."""
    k = torch.fft.fftfreq(n, d=1 / n, dtype=dtype)
    kt = torch.fft.fftfreq(nt, d=delta_t, dtype=dtype)
    kx, ky, kt = torch.meshgrid(k, k, kt, indexing="ij")
    lap = -4 * (torch.pi**2) * (kx**2 + ky**2)
    lap[0, 0] = 1
    return kx, ky, kt, lap


def residual_loss(w, psi=None, f=None, *, visc, delta_t, norm="ortho", table_dtype=None, drop=None):
    """The space-time residual of  w_t + (psi_y, -psi_x) . grad w - visc lap w - f  in Fourier space: every transform is an
    fftn / ifftn over (x, y, t); per (b, kx) the 2-norm over (ky, kt) of its real part; mean over (b, kx); / n.
    ``drop``: leave one of "time", "convection", "viscous", "forcing" out (the sensitivity check)."""
    b, n, _, nt = w.shape
    kx, ky, kt, lap = (z.to(w.device) for z in residual_tables(n, nt, delta_t, table_dtype or w.dtype))
    dims = (1, 2, 3)
    fwd = lambda z: torch.fft.fftn(z, dim=dims, norm=norm)
    inv = lambda z: torch.fft.ifftn(z, dim=dims, norm=norm)
    wh = fwd(w)
    ph = fwd(psi) if psi is not None else -wh / lap
    q = inv(2 * torch.pi * ky * 1j * ph)
    v = inv(-2.0 * torch.pi * kx * 1j * ph)
    wx = inv(2.0 * torch.pi * kx * 1j * wh)
    wy = inv(2.0 * torch.pi * ky * 1j * wh)
    terms = {"time": 2 * torch.pi * kt * 1j * wh, "convection": fwd(q * wx + v * wy), "viscous": -visc * (lap * wh)}
    if f is not None:
        terms["forcing"] = -fwd(f)
    res = sum(t for name, t in terms.items() if name != drop).real
    return torch.linalg.norm(res, dim=(-1, -2)).mean() / n


def lp_loss(x, y, d=2, p=2, h=None, size_average=True, reduction=True, relative=False):
    bsz = x.shape[0]
    diff = ((x - y).reshape(bsz, -1).abs() ** p).sum(1) ** (1 / p)
    if relative:
        out = diff / ((y.reshape(bsz, -1).abs() ** p).sum(1) ** (1 / p))
    else:
        h = 1.0 / (x.shape[1] - 1.0) if h is None else h
        out = (h ** (d / p)) * diff
    if not reduction:
        return out
    return out.mean() if size_average else out.sum()


def central_diff(u, h=None):
    """Zero-padded central differences along dims -2 and -1, (u[i+1] - u[i-1]) / 2 / h with h = 1 / n by default."""
    n = u.shape[-1]
    h = 1 / n if h is None else h
    p = torch.nn.functional.pad(u, (1, 1, 1, 1))
    gx = (p[..., 2:, 1:-1] - p[..., :-2, 1:-1]) / 2
    gy = (p[..., 1:-1, 2:] - p[..., 1:-1, :-2]) / 2
    return gx / h, gy / h


def l2_loss_2d(preds, targets, targets_grad=None, K=None, *, beta=1.0, gamma=1e-1, metric_reduction="L1", eps=1e-3, weighted=False):
    k = torch.tensor(1) if K is None else K**0.5
    tnorm = (targets**2).sum(dim=(1, 2, 3)) + eps
    if weighted:
        inv = 1 / tnorm.sqrt()
        weights = inv / inv.mean()
    else:
        weights = 1
    loss = beta * weights * ((preds - targets) ** 2).sum(dim=(1, 2, 3)) / tnorm
    if targets_grad is not None and gamma > 0:
        gnorm = 2 * (k * targets_grad**2).mean(dim=(1, 2, 3)) + eps     # the SQUARE ROOT of K here, as the reference has it
        pg = torch.cat(central_diff(preds), dim=1)
        loss = loss + gamma * ((k * (pg - targets_grad)) ** 2).mean(dim=(1, 2, 3)) / gnorm
    if metric_reduction == "L2":
        return loss.mean().sqrt()
    if metric_reduction == "L1":
        return loss.sqrt().mean()
    if metric_reduction == "Linf":
        return loss.sqrt().max()
    return loss


def bochner_norm(u, n_grid, dt=None, p=2, mesh_weighted=True, reduction=True, time_average=False, time_last=False):
    if u.ndim == 3:
        u = u.unsqueeze(0)
    if not time_last:
        u = u.permute(0, 2, 3, 1)
    ns = (u.abs() ** p).sum(dim=(1, 2)) ** (1 / p)
    ns = ns / n_grid if mesh_weighted else ns
    if time_average and dt is None:
        norm = (ns**2).mean(dim=-1).sqrt()
    elif dt is not None:
        norm = ((ns**2).sum(dim=-1) * dt).sqrt()
    else:
        raise ValueError("neither time_average nor dt")
    return norm.mean() if reduction else norm.sum()


# the small-loss cases shared by the golden script and the tests: name -> keyword arguments
LP_CASES = {f"p{p}_rel{int(rel)}_avg{int(avg)}_red{int(red)}": dict(p=p, relative=rel, size_average=avg, reduction=red)
            for p in (1, 2, 3) for rel in (False, True) for avg, red in ((True, True), (False, True), (True, False))}
LP_GRAD_CASES = ("p1_rel0_avg1_red1", "p2_rel1_avg1_red1", "p3_rel1_avg1_red1", "p3_rel0_avg0_red1")
L2_CASES = {f"{mr}_g{int(g)}_k{k}_w{int(wt)}": dict(metric_reduction=mr, with_grad=g, kmode=k, weighted=wt)
            for mr in ("L1", "L2", "Linf") for g, k, wt in ((False, 0, False), (True, 0, False), (True, 2, False), (True, 1, True))}
L2_GRAD_CASES = ("L1_g1_k2_w0", "L2_g1_k1_w1", "Linf_g0_k0_w0")
BOCHNER_CASES = {f"tl{int(tl)}_p{p}_{mode}": dict(time_last=tl, p=p, dt=(0.1 if mode == "dt" else None), time_average=(mode == "avg"))
                 for tl in (True, False) for p in (1, 2) for mode in ("dt", "avg")}
BOCHNER_GRAD_CASES = ("tl1_p1_dt", "tl0_p2_avg")
SMALL_SHAPE_TL, SMALL_SHAPE_CH = (3, 16, 16, 5), (3, 2, 16, 16)


def l2_case_inputs(kmode, dtype=torch.float64):
    preds, targets = small_inputs(SMALL_SHAPE_CH, 11, dtype=dtype)
    n, c, s, _ = SMALL_SHAPE_CH
    (tg,) = small_inputs((n, 2 * c, s, s), 12, 1, dtype=dtype)
    (kraw,) = small_inputs((n, 1, s, s), 13, 1, dtype=dtype)
    K = None if kmode == 0 else (torch.tensor(0.7, dtype=dtype) if kmode == 1 else kraw.abs() + 0.5)
    return preds, targets, tg, K


def relerr(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    den = float(torch.linalg.norm(b.reshape(-1)))
    return float(torch.linalg.norm((a.to(b.device) - b).reshape(-1))) / (den if den > 0 else 1.0)
