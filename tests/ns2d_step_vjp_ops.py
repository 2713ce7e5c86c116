"""Shared pieces of the adjoint-model tests (test-only): operators as the package builds them, seeded smooth states, tangents and
white-noise cotangents, the switch between the one-node path (``FusedSteps``) and the per-stage node chain, and the schedule
lists the goldens of tests/golden/ns2d_step_vjp.npz were made for."""
import ctypes
import functools
import math

import torch

import ns2d_ops

L = 2 * math.pi
REAL = {"f64": torch.float64, "f32": torch.float32}
CPLX = {"f64": torch.complex128, "f32": torch.complex64}
IMEX = {"imex1": (1, 1.0, 1.0), "imex1.5": (1.5, 0.5, 0.5), "imex2": (2, 0.5, 0.5)}
# golden key suffix -> (solver name, number of steps)
GOLDEN_RUNS = {"rk1": ("rk4", 1), "rk3": ("rk4", 3), "imex1": ("imex1", 2), "imex1.5": ("imex1.5", 2), "imex2": ("imex2", 2)}


def make_solver(name):
    import torch_cfd_amd as tc

    if name == "rk4":
        return tc.RK4CrankNicolsonStepper()
    order, alpha, beta = IMEX[name]
    return tc.IMEXStepper(order=order, alpha=alpha, beta=beta)


def build_op(n, tag, forcing, dev, smooth=True, solver="rk4"):
    """The operator of a case; the default dtype stays that of ``tag`` (the caller's fixture restores it)."""
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])
    forcing = None if forcing == "none" else forcing
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    fn = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False) if forcing == "kolmogorov" else None
    solver = make_solver(solver) if isinstance(solver, str) else solver
    return tc.NavierStokes2DSpectral(1e-3, grid, drag=ns2d_ops.DRAG[forcing], smooth=smooth, forcing_fn=fn, solver=solver).to(dev)


def dt_of(n):
    return 1e-3 if n <= 256 else 2.5e-4


def _smooth_fields(n, count, k0, seed):
    """`count` seeded real fields with a Gaussian spectrum of width k0 and rms 5, as fp64 half spectra."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64)
    env = torch.exp(-(k[:, None] ** 2 + k[None, : n // 2 + 1] ** 2) / (2.0 * k0 * k0))
    w = torch.fft.irfft2(torch.fft.rfft2(torch.randn(count, n, n, generator=gen, dtype=torch.float64)) * env, s=(n, n))
    return torch.fft.rfft2(5.0 * w / w.std())


@functools.lru_cache(maxsize=None)
def inputs(n, tag, B):
    """(w0, dw, g, g2) on the CPU in the precision of ``tag``: smooth vorticity fields, the half spectrum of a smooth real
    perturbation, and two white-noise complex cotangents.  Up to three distinct samples, repeated with different amplitudes."""
    k0 = min(4.0, n / 6.0)
    w0, p0 = _smooth_fields(n, min(B, 3), k0, 3000 + n), _smooth_fields(n, min(B, 3), 1.5 * k0, 4000 + n)
    reps = (B + w0.shape[0] - 1) // w0.shape[0]
    scale = (1 + 0.1 * torch.arange(B, dtype=torch.float64))[:, None, None]
    w0 = w0.repeat(reps, 1, 1)[:B] * scale
    p0 = p0.repeat(reps, 1, 1)[:B] * scale.flip(0)
    gen = torch.Generator().manual_seed(5000 + n + B)
    g = torch.view_as_complex(torch.randn(B, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64))
    g2 = torch.view_as_complex(torch.randn(B, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64))
    return tuple(x.to(CPLX[tag]).contiguous() for x in (w0, p0, g, g2))


def fields_per_chunk(op, like, batch):
    plan = op._plan(like)
    per = ctypes.c_long(0)
    assert plan.lib.tcfd_ns2d_plan_chunking(plan.handle, batch, ctypes.byref(per), None, None) == 0
    return per.value


def node_name(out):
    """Name of the autograd node that produced ``out``, looking through the reshapes / casts ``forward`` wraps it in."""
    node = out.grad_fn
    while node is not None and type(node).__name__ in ("ViewBackward0", "UnsafeViewBackward0", "ReshapeAliasBackward0", "ToCopyBackward0"):
        node = node.next_functions[0][0]
    return type(node).__name__


def grad_through_forward(op, w0, dt, steps, g, g_dwdt=None):
    """(w.grad, name of the node behind the stepped state) of  <g, w_new> [+ <g_dwdt, dwdt>]  through ``op.forward``."""
    w = w0.clone().requires_grad_(True)
    out, dwdt = op(w, dt, steps)
    loss = ns2d_ops.real_inner(g, out)
    if g_dwdt is not None:
        loss = loss + ns2d_ops.real_inner(g_dwdt, dwdt)
    name = node_name(out)
    (wbar,) = torch.autograd.grad(loss, w)
    return wbar, name
