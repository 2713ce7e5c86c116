"""Plain-torch restatement of the spectral step (test-only): the explicit terms and the generic IMEX stage loop as tensor ops
on (..., n, m) half spectra of any batch, on any device.  torch.autograd.forward_ad goes straight through it, so it serves as
the forward-mode reference for sizes and batches no golden covers (on the CPU in fp64) and as the torch-op baseline the fused
tangent step is timed against (on the GPU).  tests/test_ns2d_jvp_host.py ties it to oracle/ns2d.py and to the goldens."""
import math
from types import SimpleNamespace

import torch
import torch.autograd.forward_ad as fwAD

L = 2 * math.pi
DRAG = {None: 0.0, "none": 0.0, "kolmogorov": 0.1, "sincos": 0.0}


def tables(n, forcing=None, smooth=True, real=torch.float64, device="cpu", nu=1e-3, drag=None):
    """Constant tables of one operator (built by the oracle on the CPU in ``real``, moved to ``device``)."""
    from oracle import ns2d as O

    forcing = None if forcing == "none" else forcing
    t = O.make_tables(n, L, nu, DRAG[forcing] if drag is None else drag, smooth, None, real)
    fh = None
    if forcing == "kolmogorov":
        fh = O.kolmogorov_forcing_hat(n, L, t.kx, t.ky, 1.0, 4, False, False, real=real)
    elif forcing == "sincos":
        fh = O.sincos_forcing_hat(n, L, 0.1, 1.0, diam=L, real=real)
    t.forcing_hat = fh
    lap = O.patched_laplacian(t.kx, t.ky)
    dev = torch.device(device)
    return SimpleNamespace(n=n, real=real, kx=t.kx.to(dev), ky=t.ky.to(dev), inv_lap=(1 / lap).to(dev),
                           linear_term=t.linear_term.to(dev), mask=t.mask.to(dev) if smooth else None,
                           forcing_hat=None if fh is None else fh.to(dev), oracle=t)


def explicit_terms(w, t):
    """F(w) = mask . rfft2(-(dxw u + dyw v)) + f  (torch_cfd/equations.py:413-438)."""
    psi = -t.inv_lap * w
    two_pi_i = 2j * torch.pi
    vx, vy = torch.fft.irfft2(two_pi_i * t.ky * psi), torch.fft.irfft2(-two_pi_i * t.kx * psi)
    dx, dy = torch.fft.irfft2(two_pi_i * t.kx * w), torch.fft.irfft2(two_pi_i * t.ky * w)
    out = torch.fft.rfft2(-(dx * vx + dy * vy))
    if t.mask is not None:
        out = out * t.mask
    if t.forcing_hat is not None:
        out = out + t.forcing_hat
    return out


def schedule(stepper, dt):
    """Per-stage scalars of a stepper of the package (what the fused kernels consume)."""
    return stepper.stage_schedule(stepper.params, dt)


def step(w, t, sched):
    """One IMEX step from the per-stage scalars: h <- fa F(u) + beta h; u <- (b + gdt h + mu L b) / (1 - mud L)."""
    n = len(sched["beta"])
    fa = sched.get("fa") or [1.0] * n
    mud = sched.get("mu_den") or sched["mu"]
    base0 = sched.get("base0") or [0] * n
    start, u, h = w, w, None
    for k in range(n):
        f = explicit_terms(u, t)
        h = fa[k] * f if h is None else fa[k] * f + sched["beta"][k] * h
        b = start if base0[k] else u
        u = (b + sched["gdt"][k] * h + sched["mu"][k] * (t.linear_term * b)) / (1 - mud[k] * t.linear_term)
    return u


def advance(w, t, sched, steps=1):
    for _ in range(steps):
        w = step(w, t, sched)
    return w


def jvp(fn, w, dw):
    """(fn(w), d fn(w) . dw) by torch.autograd.forward_ad."""
    with fwAD.dual_level():
        out = fwAD.unpack_dual(fn(fwAD.make_dual(w, dw)))
        return out.primal.detach(), out.tangent.detach()


def real_inner(a, b):
    """The real inner product sum Re(conj(a) b) of two complex arrays."""
    return (a.real * b.real + a.imag * b.imag).sum()
