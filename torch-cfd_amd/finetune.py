"""The spectral refiner: fine-tuning head of the SFNO workflow (fno/finetune.py::OutConvFT).

``OutConvFT`` is the SFNO output head (``OutConv``) followed by one IMEX Crank-Nicolson pair around the predicted trajectory:
for each predicted step w, with C(.) the de-aliased convection and L the Laplacian table,

    wn(d) = (-d C(w) + d f + (1 + d nu L / 2) w) / (1 - d nu L / 2),   wt(d) = (wn(d) - w) / d           (d = -dt, +dt)
    W = a wn(-dt) + b wn(dt),   Wt = a wt(-dt) + b wt(dt),   residual = Wt + C(W) - nu L W - f        ((a, b) = bdf_weight)

and returns irfft2 of (W, Wt, residual).  The whole map, forward and backward, is one library call each
(``tcfd_ns2d_refine`` / ``tcfd_ns2d_refine_vjp``): time-last fields in, time-last fields out, no torch.fft and no host
synchronisation.  Fine-tuning trains the widened last spectral convolution on the H^-1 norm of the residual.

Numerics.  At the notebook's dt = 1e-6 the residual with bdf_weight = (0.5, 0.5) sits at the rounding floor of the
cancellation in wt(d) = (wn(d) - w) / d, about eps |w| / dt, while wt itself is O(1): errors of the residual are measured
against |w_t|.  In float32 eps / dt is about 0.1 at dt = 1e-6, so w_t carries no digits there; float32 is meant for
dt >= 1e-2.

Batches.  The reference broadcasts a forcing (b, x, y) against the (b, t, x, y / 2 + 1) spectra, which works for b = 1
only (and its (b, x, y / 2 + 1) tables for b = 1 only).  Here sample i of the batch is refined with forcing i, and
b = 1 gives the reference's result.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from .fno import OutConv, SpectralConvT

__all__ = ["OutConvFT", "refine"]


def _fft_mesh_2d(n: int, diam: float):
    k = torch.fft.fftfreq(n, d=diam / n)
    return torch.meshgrid([k, k], indexing="ij")


class _RefinePlan:
    """A ``tcfd_ns2d_plan`` whose linear term is the Laplacian table and whose mask is the de-aliasing filter, plus the
    refiner's workspace."""

    def __init__(self, n, cdtype, device, kx1, ky1, lap, mask):
        from .equations import _HipPlan

        self.hp = _HipPlan(n, cdtype, device, kx1, ky1, lap, mask)
        self.n, self.m, self.cdtype, self.rdtype, self.device = n, n // 2 + 1, cdtype, self.hp.rdtype, self.hp.device
        self._ws: Optional[torch.Tensor] = None

    def workspace(self, batch: int, nt: int) -> torch.Tensor:
        need = self.hp.lib.tcfd_ns2d_refine_workspace_bytes(self.hp.handle, batch, nt)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def rfft2(self, x):
        return self.hp.rfft2(x)

    def irfft2(self, xh):
        return self.hp.irfft2(xh)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def refine(self, w, f_hat, dt, visc, weight):
        b, nt = w.shape[0], w.shape[-1]
        outs = [torch.empty_like(w) for _ in range(3)]
        ws = self.workspace(b, nt)
        with torch.cuda.device(self.device):
            rc = self.hp.lib.tcfd_ns2d_refine(self.hp.handle, w.data_ptr(), f_hat.data_ptr() if f_hat is not None else None,
                                              *[o.data_ptr() for o in outs], b, nt, float(dt), float(visc), float(weight[0]),
                                              float(weight[1]), ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(rc, "tcfd_ns2d_refine")
        return outs

    def refine_vjp(self, w, f_hat, grads, want_f, dt, visc, weight):
        b, nt = w.shape[0], w.shape[-1]
        grad_w = torch.empty_like(w)
        grad_f = torch.empty_like(f_hat) if want_f else None
        ws = self.workspace(b, nt)
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            rc = self.hp.lib.tcfd_ns2d_refine_vjp(self.hp.handle, w.data_ptr(), ptr(f_hat), *[ptr(g) for g in grads],
                                                  grad_w.data_ptr(), ptr(grad_f), b, nt, float(dt), float(visc),
                                                  float(weight[0]), float(weight[1]), ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(rc, "tcfd_ns2d_refine_vjp")
        return grad_w, grad_f


class _RefineFn(torch.autograd.Function):
    """(w, f_hat) -> (w, w_t, residual), all real time-last (b, x, y, t); f_hat (b, x, y / 2 + 1) or None."""

    @staticmethod
    def forward(ctx, w, f_hat, plan, dt, visc, weight):
        w = w.detach().contiguous()
        fh = f_hat.detach().contiguous() if f_hat is not None else None
        ctx.plan, ctx.cfg, ctx.has_f = plan, (dt, visc, weight), f_hat is not None
        ctx.save_for_backward(w, fh) if fh is not None else ctx.save_for_backward(w)
        return tuple(plan.refine(w, fh, dt, visc, weight))

    @staticmethod
    def backward(ctx, g_w, g_wt, g_res):
        if torch.is_grad_enabled():
            # create_graph=True: the raw-pointer VJP would cut its own dependence on w out of the graph
            raise NotImplementedError("OutConvFT: double backward (create_graph=True) through the refiner is not supported")
        saved = ctx.saved_tensors
        w, fh = saved[0], (saved[1] if ctx.has_f else None)
        want_f = ctx.has_f and ctx.needs_input_grad[1]
        grads = [g.contiguous() if g is not None else None for g in (g_w, g_wt, g_res)]
        grad_w, grad_f = ctx.plan.refine_vjp(w, fh, grads, want_f, *ctx.cfg)
        return grad_w, grad_f, None, None, None, None


_PLANS: "dict[tuple, tuple]" = {}


def _refine_plan(kx, ky, lap, mask, n, cdtype, device):
    """Plan for these table tensors, resolved by identity and ``_version`` (no host copy once bound)."""
    ident = lambda t: (id(t), t.data_ptr(), t._version) if isinstance(t, torch.Tensor) else t
    key = (n, cdtype, device, ident(kx), ident(ky), ident(lap), ident(mask))
    hit = _PLANS.get(key)
    if hit is not None and all(r() is t for r, t in zip(hit[0], (kx, ky, lap, mask)) if isinstance(t, torch.Tensor)):
        return hit[1]
    m = n // 2 + 1
    first = lambda t: t.detach().reshape(-1, n, m)[0].to("cpu", torch.float64)
    kx2, ky2, lap2 = first(kx), first(ky), first(lap)
    msk = first(mask) if isinstance(mask, torch.Tensor) and mask.numel() > 1 else torch.ones(n, m, dtype=torch.float64)
    plan = _RefinePlan(n, cdtype, device, kx2[:, 0].contiguous(), ky2[0, :].contiguous(), lap2.contiguous(), msk.contiguous())
    refs = tuple(weakref.ref(t) if isinstance(t, torch.Tensor) else None for t in (kx, ky, lap, mask))
    if len(_PLANS) >= 16:
        _PLANS.pop(next(iter(_PLANS)))
    _PLANS[key] = (refs, plan)
    return plan


def refine(w, f, *, kx, ky, lap, dealias_filter, dealias, visc, dt, weight, norm="backward"):
    """``OutConvFT._fine_tune`` on the HIP kernels: w (b, x, y, t) real, f None, (x, y) or (b, x, y) real ->
    dict(w, w_t, residual), each (b, x, y, t)."""
    if not w.is_cuda:
        raise _lib.TcfdError("expected a HIP device tensor (torch-cfd_amd has no CPU fallback)")
    if norm != "backward":
        raise NotImplementedError(f"OutConvFT fine-tuning runs with norm='backward' (got {norm!r})")
    if w.dim() != 4 or w.shape[1] != w.shape[2] or w.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"expected a real (b, n, n, t) trajectory, got {tuple(w.shape)} {w.dtype}")
    b, n, _, nt = w.shape
    from .equations import _COMPLEX_OF

    cdtype = _COMPLEX_OF[w.dtype]
    mask = dealias_filter if dealias else None
    plan = _refine_plan(kx, ky, lap, mask, n, cdtype, w.device)
    f_hat = None
    if f is not None:
        from .autograd import Rfft2

        f = f.to(device=w.device, dtype=w.dtype)
        if f.dim() == 2:
            f = f.unsqueeze(0)
        f = f.expand(b, n, n) if f.shape[0] == 1 else f
        if tuple(f.shape) != (b, n, n):
            raise ValueError(f"forcing of shape {tuple(f.shape)} for a batch of {b} fields of {n} x {n}")
        f_hat = Rfft2.apply(f.contiguous(), plan.hp)
    w_, wt_, res_ = _RefineFn.apply(w, f_hat, plan, float(dt), float(visc), (float(weight[0]), float(weight[1])))
    return dict(w=w_, w_t=wt_, residual=res_)


class OutConvFT(OutConv):
    """Output head with the spectral refiner (fno/finetune.py:20-230): ``forward(v, v_res, f, out_steps)`` returns the head's
    output, or with ``finetune`` (and not ``original``) ``dict(w, w_t, residual)`` of the refiner on it."""

    def __init__(self, modes_x, modes_y, modes_t, batch_size: int = 1, diam=1.0, n_grid: int = 256, out_steps=None,
                 spatial_padding: int = 0, temporal_padding: bool = True, norm="backward", finetune=True, dealias=True,
                 delta=5e-2, visc=1e-3, dt=1e-6, bdf_weight=(0, 1), dtype=torch.float64, debug=False) -> None:
        super().__init__(modes_x=modes_x, modes_y=modes_y, modes_t=modes_t, delta=delta, n_grid=n_grid, norm=norm,
                         out_steps=out_steps, spatial_padding=spatial_padding, temporal_padding=temporal_padding)
        self.finetune = finetune
        self.out_steps = out_steps
        self.batch_size = batch_size
        self.dealias = dealias
        self.diam = diam
        self.dtype = dtype
        self.visc = visc
        self.dt = dt
        self.bdf_weight = bdf_weight
        self._initialize_fftmesh()

    def _initialize_fftmesh(self):
        """Buffers ``lap``, ``kx``, ``ky``, ``dealias_filter``, each (batch_size, n, n // 2 + 1), in the default dtype (the
        filter in ``dtype``).  The 2/3 rule compares |k| / diam with (2/3) (n // 2): all ones at diam = 2 pi."""
        kx, ky = _fft_mesh_2d(self.n_grid, self.diam)
        kmax = self.n_grid // 2
        kx, ky = [z[None].expand(self.batch_size, -1, -1)[..., : kmax + 1].contiguous() for z in (kx, ky)]
        lap = -4 * (torch.pi**2) * (abs(kx) ** 2 + abs(ky) ** 2)
        lap[..., 0, 0] = 1
        dealias_filter = (torch.logical_and(ky.abs() <= (2.0 / 3.0) * kmax, kx.abs() <= (2.0 / 3.0) * kmax).to(self.dtype)
                          if self.dealias else torch.tensor(True))
        self.register_buffer("lap", lap)
        self.register_buffer("kx", kx)
        self.register_buffer("ky", ky)
        self.register_buffer("dealias_filter", dealias_filter)

    def _update_spectral_conv_weights(self, modes_x, modes_y, modes_t, device: torch.device = None, model: nn.Module = None,
                                      debug=False):
        """Replace the head's convolution by a fresh ``SpectralConvT(1, 1, modes_x, modes_y, modes_t)`` (weights
        Xavier-uniform with gain 1e-6, zero bias) holding the old layer's blocks in its low corners: block ix + 2 iy at
        [:mx] / [-mx:] x [:my] / [-my:] x [:mt].  ``model``: the head to take the old layer from (default: self)."""
        model = self if model is None else model
        old_conv = model.conv
        conv = SpectralConvT(1, 1, modes_x, modes_y, modes_t, bias=True, delta=self.delta,
                             temporal_padding=self.temporal_padding, out_steps=self.out_steps).to(device)
        conv._reset_parameters()
        if not debug:
            mx_, my_, mt_ = old_conv.modes_x, old_conv.modes_y, old_conv.modes_t
            slice_x = [slice(0, mx_), slice(-mx_, None)]
            slice_y = [slice(0, my_), slice(-my_, None)]
            st = slice(0, mt_)
            for ix, sx in enumerate(slice_x):
                for iy, sy in enumerate(slice_y):
                    conv.weight[ix + 2 * iy].data[..., sx, sy, st, :] = old_conv.weight[ix + 2 * iy].data
                    conv.bias[ix + 2 * iy].data[..., sx, sy, st, :] = old_conv.bias[ix + 2 * iy].data
        self.conv = conv
        self.mode_x = modes_x
        self.mode_y = modes_y
        self.mode_t = modes_t

    def _fine_tune(self, w, f, **solver_kws):
        """w (b, x, y, t) -> dict(w, w_t, residual), each (b, x, y, t); f None (zero forcing) or (b, x, y)."""
        return refine(w, f, kx=self.kx, ky=self.ky, lap=self.lap, dealias_filter=self.dealias_filter, dealias=self.dealias,
                      visc=self.visc, dt=self.dt, weight=self.bdf_weight, norm=self.norm)

    def forward(self, v, v_res, f=None, out_steps: int = None, original=False):
        """v: latent (b, 1, x, y, t_latent); v_res: input (b, x, y, t_in); f: forcing (b, x, y) or None."""
        v = super().forward(v, v_res, out_steps=out_steps)
        if not self.finetune or original:
            return v
        return self._fine_tune(v, f)
