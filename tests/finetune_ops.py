"""Torch-ops restatement of the spectral refiner (fno/finetune.py::OutConvFT._fine_tune with the legacy IMEX step and
residual of fno/data_gen/solvers.py), differentiable by torch autograd, for the GPU tests and tests/bench_finetune.py.  It
runs on any device through torch.fft; nothing in it calls the library.  Also the smooth test trajectories of the goldens."""
import math

import torch


def tables(n, diam, batch=1, dealias=True, dtype=None):
    """(kx, ky, lap, mask) as OutConvFT builds them: (batch, n, n // 2 + 1) in the default dtype."""
    k = torch.fft.fftfreq(n, d=diam / n)
    kx, ky = torch.meshgrid([k, k], indexing="ij")
    kmax = n // 2
    kx, ky = [z[None].expand(batch, -1, -1)[..., : kmax + 1].contiguous() for z in (kx, ky)]
    lap = -4 * (torch.pi**2) * (abs(kx) ** 2 + abs(ky) ** 2)
    lap[..., 0, 0] = 1
    mask = (torch.logical_and(ky.abs() <= (2.0 / 3.0) * kmax, kx.abs() <= (2.0 / 3.0) * kmax).to(dtype or kx.dtype)
            if dealias else None)
    return kx, ky, lap, mask


def convection(w_h, kx, ky, lap, mask):
    n = w_h.shape[-2]
    psi = -w_h / lap
    u = 2 * math.pi * ky * 1j * psi
    v = -2.0 * math.pi * kx * 1j * psi
    wx = 2.0 * math.pi * kx * 1j * w_h
    wy = 2.0 * math.pi * ky * 1j * w_h
    u, v, wx, wy = [torch.fft.irfft2(z, s=(n, n)).real for z in (u, v, wx, wy)]
    c = torch.fft.rfft2(u * wx + v * wy)
    return mask * c if mask is not None else c


def refine_ops(w, f, kx, ky, lap, mask, visc, dt, weight):
    """w (b, x, y, t) real, f None or (b, x, y) -> dict(w, w_t, residual); sample i uses forcing i."""
    b, n, _, nt = w.shape
    wf = w.permute(0, 3, 1, 2)
    kx, ky, lap = [z.reshape(-1, n, n // 2 + 1)[:1].to(device=w.device) for z in (kx, ky, lap)]
    kxc, kyc = kx.to(torch.complex128 if w.dtype == torch.float64 else torch.complex64), None
    kyc = ky.to(kxc.dtype)
    lap = lap.to(w.dtype)
    mask = mask.reshape(-1, n, n // 2 + 1)[:1].to(device=w.device) if mask is not None else None
    w_h = torch.fft.rfftn(wf, s=(n, n))
    f_h = torch.fft.rfftn(f.to(w.dtype), s=(n, n))[:, None] if f is not None else torch.zeros_like(w_h)
    conv1 = convection(w_h, kxc, kyc, lap, mask)
    wn, wt = [], []
    for d in (-dt, dt):
        nxt = (-d * conv1 + d * f_h + (1.0 + 0.5 * d * visc * lap) * w_h) / (1.0 - 0.5 * d * visc * lap)
        wn.append(nxt)
        wt.append((nxt - w_h) / d)
    W = weight[0] * wn[0] + weight[1] * wn[1]
    Wt = weight[0] * wt[0] + weight[1] * wt[1]
    res = Wt + convection(W, kx.to(w.dtype), ky.to(w.dtype), lap, mask) - visc * lap * W - f_h
    out = [torch.fft.irfftn(z, s=(n, n)).real.permute(0, 2, 3, 1) for z in (W, Wt, res)]
    return dict(w=out[0], w_t=out[1], residual=out[2])


def smooth_trajectory(batch, n, nt, dtype=torch.float64, phase=0.0):
    """A smooth (b, n, n, nt) vorticity trajectory: a few Fourier modes with time-varying amplitudes (no random numbers)."""
    x = torch.arange(n, dtype=torch.float64) / n
    X, Y = torch.meshgrid(x, x, indexing="ij")
    modes = ((1, 0, 1.0), (0, 1, -0.8), (1, 1, 0.6), (2, -1, 0.4), (3, 2, 0.25), (-4, 1, 0.15), (5, 5, 0.05))
    out = torch.zeros(batch, n, n, nt, dtype=torch.float64)
    for s in range(batch):
        for t in range(nt):
            acc = torch.zeros(n, n, dtype=torch.float64)
            for j, (kx, ky, a) in enumerate(modes):
                amp = a * (1.0 + 0.1 * t + 0.05 * s * (j + 1))
                acc = acc + amp * torch.cos(2 * math.pi * (kx * X + ky * Y) + 0.3 * j + phase + 0.7 * s)
            out[s, :, :, t] = acc
    return out.to(dtype)


def smooth_forcing(batch, n, dtype=torch.float64):
    x = torch.arange(n, dtype=torch.float64) / n
    X, Y = torch.meshgrid(x, x, indexing="ij")
    f = torch.stack([0.1 * (torch.sin(2 * math.pi * (X + Y)) + torch.cos(2 * math.pi * (X + Y))) * (1 + 0.5 * s)
                     + 0.05 * torch.cos(8 * math.pi * Y) for s in range(batch)])
    return f.to(dtype)
