"""Plain-torch restatement of the finite-volume step (test-only): the same operation order as the HIP kernels and the
reference (torch_cfd/fvm.py, interpolation.py, finite_differences.py, pressure.py), on (..., n, n) tensors of any batch.
It lets GPU tests check sizes and batches no golden covers; tests/test_fvm_host.py checks it against the goldens."""
import math

import torch


def _sh(x, k, axis):
    """x.shift(k, axis): entry i holds x[i + k] (periodic)."""
    return torch.roll(x, -k, dims=axis)


def _half(a, b):
    return 0.5 * a + 0.5 * b


def _tvd_flux(cm, c0, c1, c2, w, cfl):
    pos = w > 0
    clow = torch.where(pos, c0, c1)
    cr = cfl * w
    d = c1 - c0
    hp = c0 + 0.5 * (1 - cr) * d
    hn = c1 - 0.5 * (1 + cr) * d
    chigh = torch.where(pos, hp, hn)
    dd = torch.where(d != 0, d, torch.ones_like(d))

    def lim(r):
        rp1 = 1 + r
        return torch.where(r > 0, (2 * r) / torch.where(rp1 != 0, rp1, torch.ones_like(rp1)), torch.zeros_like(r))

    phi = torch.where(pos, lim((c0 - cm) / dd), lim((c2 - c1) / dd))
    return (clow - (clow - chigh) * phi) * w


def _advect(c, wx, wy, cfl, h):
    ax, ay = -2, -1
    fx = _tvd_flux(_sh(c, -1, ax), c, _sh(c, 1, ax), _sh(c, 2, ax), wx, cfl)
    fy = _tvd_flux(_sh(c, -1, ay), c, _sh(c, 1, ay), _sh(c, 2, ay), wy, cfl)
    return -((fx - _sh(fx, -1, ax)) / h + (fy - _sh(fy, -1, ay)) / h)


def laplacian(u, h):
    s = 1 / h**2
    out = -2 * u * (s + s)
    out = out + (_sh(u, -1, -2) + _sh(u, 1, -2)) * s
    return out + (_sh(u, -1, -1) + _sh(u, 1, -1)) * s


def explicit_terms(ux, uy, dt, h, nu, drag=0.0, force=None):
    """du/dt of the staggered pair: van Leer advection + nu lap + force - drag u (force: (fx, fy) already / density)."""
    cfl = dt / h
    conv_x = _advect(ux, _half(ux, _sh(ux, 1, -2)), _half(uy, _sh(uy, 1, -2)), cfl, h)
    conv_y = _advect(uy, _half(ux, _sh(ux, 1, -1)), _half(uy, _sh(uy, 1, -1)), cfl, h)
    kx = conv_x + nu * laplacian(ux, h)
    ky = conv_y + nu * laplacian(uy, h)
    if force is not None:
        kx = kx + force[0]
        ky = ky + force[1]
    if drag > 0:
        kx = kx + ux * -drag
        ky = ky + uy * -drag
    return kx, ky


def inverse_eigenvalues(n, h, dtype=torch.float64):
    col = torch.zeros(n, dtype=dtype)
    col[0] = -2 / h**2
    col[1] = col[-1] = 1 / h**2
    lam = torch.fft.fft(col)[:, None] + torch.fft.rfft(col)[None, :]
    return torch.where(torch.abs(lam) > 10 * torch.finfo(torch.float32).eps, 1 / lam, 0)


def project(ux, uy, h, inverse):
    div = (ux - _sh(ux, -1, -2)) / h + (uy - _sh(uy, -1, -1)) / h
    q = torch.fft.irfft2(inverse * torch.fft.rfft2(div), s=div.shape[-2:])
    return ux - (_sh(q, 1, -2) - q) / h, uy - (_sh(q, 1, -1) - q) / h


def step(ux, uy, dt, a, b, h, nu, drag=0.0, force=None, inverse=None):
    """One RK step; a (stages x stages row-major) and b are the increments' weights dt * a_ij, dt * b_j (0: skipped)."""
    s = len(b)
    if inverse is None:
        inverse = inverse_eigenvalues(ux.shape[-1], h).to(ux.device)
    ks = []
    cur = (ux, uy)
    for i in range(s):
        if i > 0:
            px, py = ux, uy
            for j in range(i):
                if a[i * s + j] != 0:
                    px = px + a[i * s + j] * ks[j][0]
                    py = py + a[i * s + j] * ks[j][1]
            cur = project(px, py, h, inverse)
        ks.append(explicit_terms(cur[0], cur[1], dt, h, nu, drag, force))
    px, py = ux, uy
    for j in range(s):
        if b[j] != 0:
            px = px + b[j] * ks[j][0]
            py = py + b[j] * ks[j][1]
    return project(px, py, h, inverse)


def kolmogorov_staggered(n, wave, scale=1.0, L=2 * math.pi, dtype=torch.float64):
    """Kolmogorov forcing sampled at the staggered faces: fx = sin(k y) at y = (j + 1/2) h, fy = 0."""
    h = L / n
    y = (torch.arange(n, dtype=dtype) + 0.5) * h
    fx = scale * torch.sin(wave * (2 * math.pi / L) * y)[None, :].expand(n, n).contiguous()
    return fx, torch.zeros_like(fx)
