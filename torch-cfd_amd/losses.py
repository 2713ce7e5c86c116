"""Fourier-domain Sobolev loss of the SFNO training path (reference: fno/losses.py:199-315) on the HIP kernels of
csrc/tcfd_loss.hip: the forward value in three launches on the time-last tensors in place, and -- under autograd -- its gradient with
respect to the prediction in three more (``tcfd_sobolev_loss_backward``).  Shapes outside the fused kernels' cover compose the loss
from the HIP rfft2 (``autograd.Rfft2``) and a one-pass weighted reduction."""
import ctypes
import math
import os
from typing import Dict

import torch
import torch.nn as nn

from . import _lib
from .autograd import Rfft2 as _Rfft2Fn   # rfft2 on the HIP kernels with its hand-written adjoint

_LOSS_PLANS: Dict[tuple, ctypes.c_void_p] = {}   # (n, precision, device) -> tcfd_loss_plan (a twiddle table; lives with the process)


def hip_weighted_sqnorm(zh: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """``(|zh|^2 * w2).sum(dim=(-2, -1))`` for half spectra ``zh`` (*, n, m) and real weights ``w2`` (n, m) in one pass
    over the spectrum (``tcfd_weighted_sqnorm``; double accumulation, the result comes back in ``w2.dtype``)."""
    if not zh.is_cuda:
        raise _lib.TcfdError("expected a HIP device tensor (torch-cfd_amd has no CPU fallback)")
    lead, elems = zh.shape[:-2], zh.shape[-2] * zh.shape[-1]
    if tuple(w2.shape) != tuple(zh.shape[-2:]):
        raise ValueError(f"weights {tuple(w2.shape)} for spectra {tuple(zh.shape[-2:])}")
    cdt = zh.dtype
    rdt = torch.float64 if cdt == torch.complex128 else torch.float32
    zc = zh.contiguous()
    wc = w2.to(device=zh.device, dtype=rdt).contiguous()
    batch = max(int(zc.numel() // elems), 1)
    blocks = max(1, min(64, (elems + 4095) // 4096))
    partial = torch.empty(batch, blocks, dtype=torch.float64, device=zh.device)
    with torch.cuda.device(zh.device):
        _lib.check(_lib.load().tcfd_weighted_sqnorm(
            zc.data_ptr(), wc.data_ptr(), partial.data_ptr(), batch, elems, blocks,
            _lib.TCFD_C128 if cdt == torch.complex128 else _lib.TCFD_C64,
            ctypes.c_void_p(torch.cuda.current_stream(zh.device).cuda_stream)), "tcfd_weighted_sqnorm")
    return partial.sum(dim=-1).to(w2.dtype).reshape(lead)


def _fused_forward(plan, xc, yc, w2, ws, flags, sums):
    """``tcfd_sobolev_loss`` on contiguous time-last tensors; ``sums``: (nfields, batch, nt) doubles kept for the backward pass."""
    nf, relative, mesh, tavg, red = flags
    bsz, nt = xc.shape[0], xc.shape[-1]
    out = torch.empty((), dtype=xc.dtype, device=xc.device)
    with torch.cuda.device(xc.device):
        _lib.check(_lib.load().tcfd_sobolev_loss(plan, xc.data_ptr(), yc.data_ptr() if yc is not None else None, w2.data_ptr(), bsz, nt,
                                                 nf, relative, mesh, tavg, red, out.data_ptr(),
                                                 sums.data_ptr() if sums is not None else None, ws.data_ptr(), ws.numel(),
                                                 ctypes.c_void_p(torch.cuda.current_stream(xc.device).cuda_stream)), "tcfd_sobolev_loss")
    return out


class _FusedLossFn(torch.autograd.Function):
    """The fused loss as one autograd node: forward = the three launches of ``tcfd_sobolev_loss`` (per-time sums kept), backward =
    the three of ``tcfd_sobolev_loss_backward`` -- d = x - y is transformed again rather than 94 MB of half spectra kept across
    the training step.  Replaces (round 4) two permuted copies, an rfft2 with its adjoint and eight elementwise kernels over the
    spectrum: 0.9 -> 0.3 ms of a config-5 training step."""

    @staticmethod
    def forward(ctx, x, yc, plan, w2, wf, ws, flags, module):
        xc = x.detach()           # contiguous: SobolevLoss._fused hands over the contiguous form (a view of the caller's tensor when it is)
        sums = torch.empty(flags[0] * xc.shape[0] * xc.shape[-1], dtype=torch.float64, device=xc.device)
        out = _fused_forward(plan, xc, yc, w2, ws, flags, sums)
        # x itself, not its detached twin: a backward pass under create_graph=True differentiates through it again
        ctx.save_for_backward(x, yc if yc is not None else xc.new_empty(0), wf, sums)
        ctx.cfg = (plan, ws, flags, yc is not None, module)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, yc, wf, sums = ctx.saved_tensors
        plan, ws, flags, has_y, module = ctx.cfg
        if torch.is_grad_enabled():
            # create_graph=True (gradient penalties, Hessian-vector products through the loss): the raw-pointer launches below
            # would return a constant.  Form the gradient from the composed loss -- Rfft2 (autograd.py, differentiable any number
            # of times) plus tensor operations -- as FusedExplicitTerms.backward does for the solver, and as the reference's
            # pure-torch loss allows (fno/losses.py:263-315).
            with torch.enable_grad():
                xin = x if x.requires_grad else x.detach().requires_grad_(True)
                loss = module._composed(xin, yc if has_y else None)
                (grad,) = torch.autograd.grad(loss, xin, gout.to(loss.dtype), create_graph=True)
            return grad, None, None, None, None, None, None, None
        xc = x.detach()
        nf, relative, mesh, tavg, red = flags
        g = gout.detach().to(xc.dtype).contiguous()
        grad = torch.empty_like(xc)
        with torch.cuda.device(xc.device):
            _lib.check(_lib.load().tcfd_sobolev_loss_backward(
                plan, xc.data_ptr(), yc.data_ptr() if has_y else None, wf.data_ptr(), sums.data_ptr(), g.data_ptr(), xc.shape[0],
                xc.shape[-1], nf, relative, mesh, tavg, red, grad.data_ptr(), ws.data_ptr(), ws.numel(),
                ctypes.c_void_p(torch.cuda.current_stream(xc.device).cuda_stream)), "tcfd_sobolev_loss_backward")
        return grad, None, None, None, None, None, None, None


# workspaces of the fused loss, per (device, bytes needed rounded up): outside the modules (a device tensor in a plain module
# attribute rides along with copy.deepcopy / torch.save(module), is not moved by .to() and would pin a CUDA graph's private pool
# if first allocated during capture)
_LOSS_WORKSPACES: Dict[torch.device, torch.Tensor] = {}


def _loss_workspace(device: torch.device, need: int) -> torch.Tensor:
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)     # belongs to the capture, never cached
    ws = _LOSS_WORKSPACES.get(device)
    if ws is None or ws.numel() < need:
        _LOSS_WORKSPACES.pop(device, None)
        ws = _LOSS_WORKSPACES[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


class SobolevLoss(nn.Module):
    """Fourier-domain weighted norm of (x - y), fno/losses.py:199-315, including ``freq_cutoff`` (wavenumbers above it
    are replaced by inf for negative orders and by 0 otherwise, exactly as the reference's mesh does) and every
    ``fft_norm``.

    Copies the code's behaviour, not its comment: for ``norm_order == 0`` the multiplier is
    sqrt(alpha + 4 pi^2 |k|^2) itself, not 1.  The 2-D transforms over dims (1, 2) of the
    time-last tensors run on the HIP rfft2 kernels (one Hermitian-weighted half spectrum per time slice
    instead of the reference's full complex fftn); everything else is a handful of device reductions."""

    def __init__(self, n_grid: int = 256, time_average: bool = True, reduction: bool = True, mesh_weighted: bool = True,
                 relative: bool = False, inp_time_last: bool = True, freq_cutoff: int = None, norm_order: float = -1,
                 alpha: float = 0.1, fft_norm: str = "backward", diam: float = 1, debug: bool = False):
        super().__init__()
        if fft_norm not in (None, "backward", "ortho", "forward"):
            raise ValueError(f"unknown fft norm {fft_norm!r}")
        # |fftn(z, norm)|^2 = |fftn(z)|^2 / n^2 ("ortho") or / n^4 ("forward"): a scalar on the squared norms
        self.fft_norm = fft_norm
        self._sq_scale = {None: 1.0, "backward": 1.0, "ortho": 1.0 / n_grid**2, "forward": 1.0 / n_grid**4}[fft_norm]
        self.relative, self.time_average, self.reduction = relative, time_average, reduction
        self.mesh_weighted, self.norm_order, self.alpha = mesh_weighted, norm_order, alpha
        self.inp_time_last, self.n_grid, self.diam = inp_time_last, n_grid, diam
        n = n_grid
        k = torch.fft.fftfreq(n, d=diam / n)
        kx, ky = torch.meshgrid([k, k], indexing="ij")
        cutoff = (n // 2 + 1 if freq_cutoff is None else freq_cutoff) / diam
        fill = math.inf if norm_order < 0 else 0.0
        kx = kx.clone().masked_fill(kx.abs() > cutoff, fill)
        ky = ky.clone().masked_fill(ky.abs() > cutoff, fill)
        weight = alpha + 4 * (torch.pi) ** 2 * (kx**2 + ky**2)
        self.register_buffer("kx", kx[None, :, :, None])
        self.register_buffer("ky", ky[None, :, :, None])
        self.register_buffer("weight", weight[None, :, :, None])

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_w2_cache", None)      # a device-side table rebuilt on demand: not part of a pickled / deep-copied module
        return state

    def _half_spectrum_weights(self, device, dtype):
        """(n, n/2+1) table: multiplier^2 x Hermitian multiplicity x fft-norm scale.  Built once per (device, dtype) and
        state of the ``weight`` buffer -- it took ~20 small launches per call, more than the loss kernels themselves."""
        key = (torch.device(device), dtype, self.weight.data_ptr(), self.weight._version, self.norm_order, self._sq_scale)
        cached = self.__dict__.get("_w2_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        n = self.n_grid
        # sqrt and power in the BUFFER's precision, as the reference forms its multiplier (losses.py:279-289) before the
        # product with the spectrum promotes it: a float32 module on float64 data uses float32-rounded weights there too
        # (and on the CPU, once: a device pow differs from the CPU's in the last float32 bit, 5e-10 on an order -1 loss)
        w = torch.sqrt(self.weight[0, :, : n // 2 + 1, 0].detach().cpu())
        w = (w ** (self.norm_order / 2) if self.norm_order != 0 else w).to(device=device, dtype=dtype)
        herm = torch.full((n // 2 + 1,), 2.0, dtype=dtype, device=device)  # |X[k]|^2 counted twice except DC/Nyquist
        herm[0] = 1.0
        herm[-1] = 1.0
        w2 = (w**2 * herm * self._sq_scale).contiguous()
        self._w2_cache = (key, w2, (w**2 * self._sq_scale).contiguous())    # ... and without the multiplicity (backward pass)
        return w2

    def _fused(self, x, y):
        """The loss in three launches on the time-last tensors in place (``tcfd_sobolev_loss``, csrc/tcfd_loss.hip), or None
        when this call is outside its cover (a target that needs a gradient, a grid off the FFT kernels -- 2^k in [16, 1024],
        3 * 2^k in [96, 768], 5 * 2^k in [80, 640] --, more time steps than one workgroup transforms).  With a prediction that
        needs a gradient the same kernels run inside ``_FusedLossFn``, whose backward is ``tcfd_sobolev_loss_backward``."""
        if os.environ.get("TCFD_LOSS_FUSED", "1") == "0" or not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
            return None
        wants_grad = torch.is_grad_enabled() and x.requires_grad
        if torch.is_grad_enabled() and y is not None and y.requires_grad:
            return None                                   # a target that needs a gradient: the composed path below
        if wants_grad and os.environ.get("TCFD_LOSS_FUSED_BWD", "1") == "0":
            return None
        bsz, n, n2, nt = x.shape
        if (n != n2 or not ((16 <= n <= 1024 and (n & (n - 1)) == 0) or n in (96, 192, 384, 768, 80, 160, 320, 640)) or bsz == 0
                or (y is not None and (y.shape != x.shape or y.dtype != x.dtype))):
            return None
        lib = _lib.load()
        code = _lib.TCFD_C128 if x.dtype == torch.float64 else _lib.TCFD_C64
        pkey = (n, code, x.device)
        plan = _LOSS_PLANS.get(pkey)
        if plan is None:
            handle = ctypes.c_void_p()
            with torch.cuda.device(x.device):
                _lib.check(lib.tcfd_loss_plan_create(ctypes.byref(handle), n, code), "tcfd_loss_plan_create")
            plan = _LOSS_PLANS[pkey] = handle
        nf = 2 if (self.relative and y is not None) else 1
        if not lib.tcfd_sobolev_loss_supported(plan, nt, nf):
            return None
        xc = x.contiguous()
        yc = y.contiguous() if y is not None else None
        w2 = self._half_spectrum_weights(x.device, x.dtype)
        ws = _loss_workspace(x.device, lib.tcfd_loss_workspace_bytes(plan, bsz, nt, nf))
        flags = (nf, int(bool(self.relative and y is not None)),
                 (2 if torch.get_default_dtype() == torch.float32 else 1) if self.mesh_weighted else 0,
                 int(bool(self.time_average)), int(bool(self.reduction)))
        if wants_grad:
            return _FusedLossFn.apply(xc, yc, plan, w2, self._w2_cache[2], ws, flags, self)
        return _fused_forward(plan, xc, yc, w2, ws, flags, None)

    def forward(self, x, y=None):
        if not self.inp_time_last:
            x = x.permute(0, 2, 3, 1)
            y = y.permute(0, 2, 3, 1) if y is not None else None
        bsz, n, _, nt = x.shape
        if n != self.n_grid:
            raise ValueError(f"grid {n} != n_grid {self.n_grid}")
        # relative loss without a target: the reference divides by the norm of its all-zero y (losses.py:283-299) -- inf (nan
        # for x = 0), reproduced by dividing the plain norm by zero
        no_target = 0.0 if (self.relative and y is None) else None
        fused = self._fused(x, y)
        if fused is not None:
            return fused if no_target is None else fused / no_target
        loss = self._composed(x, y)
        return loss if no_target is None else loss / no_target

    def _composed(self, x, y=None):
        """The loss of time-last x (and y) composed from the HIP rfft2 (``autograd.Rfft2`` under autograd: differentiable any
        number of times) and tensor operations: what runs outside the fused kernels' cover, and what the fused node's backward
        differentiates when a graph of the gradient itself is asked for."""
        from .equations import fft_plan

        bsz, n, _, nt = x.shape
        plan = fft_plan(n, torch.complex64 if x.dtype == torch.float32 else torch.complex128, x.device, self.diam)
        w2 = self._half_spectrum_weights(x.device, x.dtype)

        def sq_norms(z):  # (b, n, n, t) -> (b, t): || w * fft2(z_t) ||_F^2 via the half spectrum
            zt = z.permute(0, 3, 1, 2).contiguous()
            if torch.is_grad_enabled() and zt.requires_grad:
                zh = _Rfft2Fn.apply(zt, plan)
                return ((zh.real**2 + zh.imag**2) * w2).sum(dim=(-2, -1))
            zh = plan.rfft2(zt)
            return hip_weighted_sqnorm(zh, w2)

        diff = sq_norms(x if y is None else x - y)  # the transform is linear: one rfft2 of the difference
        loss = diff.sum(dim=-1).sqrt()
        if self.relative and y is not None:
            yn = sq_norms(y).sum(dim=-1).sqrt()
        else:
            # the reference's unit norms are torch.ones(bsz) in the DEFAULT dtype (losses.py:297): under a float32 default, 1 / n
            # is rounded to float32 before it divides a float64 loss (1.5e-8 at n = 80; exact when n is a power of two)
            yn = torch.ones(bsz, device=x.device, dtype=torch.get_default_dtype())
        yn = (yn / n if self.mesh_weighted else yn).to(x.dtype)
        loss = loss / yn
        loss = loss / math.sqrt(nt) if self.time_average else loss
        loss = loss.mean(0) if self.reduction else loss.sum(0)
        return loss / n if self.mesh_weighted else loss


# ===================================================================================================================
# The other losses of fno/losses.py: LpLoss, L2Loss2d (+ central_diff), BochnerNorm and ResidualLoss on the kernels of
# csrc/tcfd_residual.hip.  Workspaces come from the caching allocator per call (stream-ordered: nothing is shared across streams).
def _code(dtype):
    return _lib.TCFD_C128 if dtype == torch.float64 else _lib.TCFD_C64


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_hip(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.TcfdError("expected a HIP device tensor (torch-cfd_amd has no CPU fallback)")


def _lp_sums_ops(x, y, outer, reduce, inner, p, want_y):
    """``tcfd_lp_sums`` in tensor operations (float64 sums): differentiable any number of times."""
    d = (x if y is None else x - y).reshape(outer, reduce, inner).double()
    sd = (d.abs() ** p).sum(1)
    sy = (y.reshape(outer, reduce, inner).double().abs() ** p).sum(1) if want_y else sd.new_zeros(outer, inner)
    return sd, sy


class _LpSumsFn(torch.autograd.Function):
    """sum |x - y|^p and sum |y|^p over the middle axis of the (outer, reduce, inner) view: ``tcfd_lp_sums`` forward (one pass,
    double accumulators, two fixed-order stages), ``tcfd_lp_sums_bwd`` backward (one elementwise pass)."""

    @staticmethod
    def forward(ctx, x, y, outer, reduce, inner, p, want_y):
        xc = x.detach().contiguous()
        yc = y.detach().contiguous() if y is not None else None
        lib = _lib.load()
        sd = torch.empty(outer, inner, dtype=torch.float64, device=x.device)
        sy = torch.empty(outer, inner, dtype=torch.float64, device=x.device) if want_y else None
        ws = torch.empty(lib.tcfd_lp_sums_workspace_bytes(outer, reduce, inner), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.tcfd_lp_sums(xc.data_ptr(), yc.data_ptr() if yc is not None else None, sd.data_ptr(),
                                        sy.data_ptr() if want_y else None, outer, reduce, inner, float(p), _code(x.dtype),
                                        ws.data_ptr(), ws.numel(), _stream_ptr(x.device)), "tcfd_lp_sums")
        ctx.save_for_backward(x, y if y is not None else x.new_empty(0))
        ctx.cfg = (outer, reduce, inner, p, want_y, y is not None)
        if not want_y:
            sy = sd.new_zeros(outer, inner)
            ctx.mark_non_differentiable(sy)
        return sd, sy

    @staticmethod
    def backward(ctx, gd, gy):
        x, y = ctx.saved_tensors
        outer, reduce, inner, p, want_y, has_y = ctx.cfg
        y = y if has_y else None
        need_x, need_y = ctx.needs_input_grad[0], has_y and ctx.needs_input_grad[1]
        if torch.is_grad_enabled():        # create_graph=True: differentiate the tensor-op form
            with torch.enable_grad():
                xin = x if x.requires_grad else x.detach().requires_grad_(True)
                yin = (y if y.requires_grad else y.detach().requires_grad_(True)) if need_y else y
                sd, sy = _lp_sums_ops(xin, yin, outer, reduce, inner, p, want_y)
                total = (sd * gd).sum() + ((sy * gy).sum() if (want_y and gy is not None) else 0)
                gs = torch.autograd.grad(total, [xin] + ([yin] if need_y else []), create_graph=True, allow_unused=True)
            return (gs[0] if need_x else None), (gs[1] if need_y else None), None, None, None, None, None
        xc = x.detach().contiguous()
        yc = y.detach().contiguous() if has_y else None
        cd = gd.detach().to(torch.float64).contiguous()
        cy = gy.detach().to(torch.float64).contiguous() if (want_y and gy is not None) else None
        gx = torch.empty_like(xc) if need_x else None
        gyy = torch.empty_like(yc) if need_y else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().tcfd_lp_sums_bwd(xc.data_ptr(), yc.data_ptr() if has_y else None, cd.data_ptr(),
                                                    cy.data_ptr() if cy is not None else None, gx.data_ptr() if need_x else None,
                                                    gyy.data_ptr() if need_y else None, outer, reduce, inner, float(p),
                                                    _code(x.dtype), _stream_ptr(x.device)), "tcfd_lp_sums_bwd")
        return (gx.reshape(x.shape) if need_x else None), (gyy.reshape(y.shape) if need_y else None), None, None, None, None, None


def hip_lp_sums(x, y, outer, reduce, inner, p, want_y=False):
    """(sum |x - y|^p, sum |y|^p) over the middle axis of the contiguous (outer, reduce, inner) view, float64, shape
    (outer, inner); ``y`` may be None.  The kernel takes finite p > 0, float32 / float64, inner <= 256, outer <= 65535;
    anything else raises ``ValueError`` (the callers route those to tensor operations)."""
    _need_hip(x, y)
    if (x.dtype not in (torch.float32, torch.float64) or (y is not None and (y.dtype != x.dtype or y.shape != x.shape))
            or not (0 < p < math.inf) or inner > 256 or outer > 65535 or x.numel() != outer * reduce * inner or x.numel() == 0):
        raise ValueError("hip_lp_sums: outside the kernel's cover")
    return _LpSumsFn.apply(x, y, int(outer), int(reduce), int(inner), float(p), bool(want_y))


def _lp_kernel_ok(x, y, p, inner=1, outer=1):
    return (x.is_cuda and x.dtype in (torch.float32, torch.float64) and (y is None or (y.dtype == x.dtype and y.shape == x.shape))
            and isinstance(p, (int, float)) and 0 < p < math.inf and inner <= 256 and outer <= 65535 and x.numel() > 0)


class LpLoss(nn.Module):
    """Relative / absolute Lp loss of the FNO baselines, fno/losses.py:140-196: per sample ||x - y||_p over everything but the
    batch, ``abs`` scaled by h^(d/p) (h = 1 / (x.size(1) - 1) unless given), ``rel`` divided by ||y||_p; mean, sum or the
    per-sample vector.  One pass over x and y (``tcfd_lp_sums``); p = inf goes through torch.linalg.norm."""

    def __init__(self, d=2, p=2, h=None, size_average=True, reduction=True, relative=False):
        super().__init__()
        assert d > 0 and p > 0
        self.d, self.p, self.h = d, p, h
        self.reduction, self.size_average, self.relative = reduction, size_average, relative

    def _norms(self, x, y, want_y):
        _need_hip(x, y)
        bsz = x.size(0)
        if not _lp_kernel_ok(x, y, self.p, 1, bsz):
            diff = torch.linalg.norm(x.reshape(bsz, -1) - y.reshape(bsz, -1), self.p, 1)
            return diff, (torch.linalg.norm(y.reshape(bsz, -1), self.p, 1) if want_y else None)
        sd, sy = hip_lp_sums(x, y, bsz, x.numel() // bsz, 1, self.p, want_y)
        root = 1.0 / self.p
        return (sd[:, 0] ** root).to(x.dtype), ((sy[:, 0] ** root).to(x.dtype) if want_y else None)

    def _reduce(self, v):
        if self.reduction:
            return torch.mean(v) if self.size_average else torch.sum(v)
        return v

    def abs(self, x, y):
        h = 1.0 / (x.size(1) - 1.0) if self.h is None else self.h
        diff, _ = self._norms(x, y, False)
        return self._reduce((h ** (self.d / self.p)) * diff)

    def rel(self, x, y):
        diff, yn = self._norms(x, y, True)
        return self._reduce(diff / yn)

    def forward(self, x, y):
        return self.rel(x, y) if self.relative else self.abs(x, y)


def central_diff(u: torch.Tensor, h: float = None, mode="constant", padding=True, value=None, channel_last=False):
    """fno/losses.py:10-47: central differences (u[i+1] - u[i-1]) / 2 / h along the two spatial dims of (b, n, n),
    (b, C, n, n), (b, T, C, n, n) (``channel_last``: (b, n, n, C), (b, T, n, n, C)), padded by one point (zeros by default);
    h = 1 / n unless given.  Tensor operations (``L2Loss2d`` fuses the same stencil into its H^1 kernel)."""
    bsz, *sizes = u.shape
    n = sizes[1] if channel_last else sizes[-1]
    h = 1 / n if h is None else h
    if channel_last:
        u = u.transpose(-1, -3)
    if padding:
        u = torch.nn.functional.pad(u, (1, 1, 1, 1), mode=mode, value=value)
    d, s = 2, 1
    gradx = (u[..., d:, s:-s] - u[..., :-d, s:-s]) / d
    grady = (u[..., s:-s, d:] - u[..., s:-s, :-d]) / d
    if channel_last:
        gradx, grady = gradx.transpose(-3, -1), grady.transpose(-3, -1)
    return gradx / h, grady / h


def _h1_sums_ops(preds, tgrad, ksqrt, h):
    gx, gy = central_diff(preds, h=h)
    k = 1 if ksqrt is None else ksqrt
    s1 = ((k * (torch.cat([gx, gy], dim=1) - tgrad)).double() ** 2).sum(dim=(1, 2, 3))
    s2 = (k * tgrad**2).double().expand(tgrad.shape).sum(dim=(1, 2, 3))
    return s1, s2


class _H1SumsFn(torch.autograd.Function):
    """Per sample: sum (ksqrt (central_diff(preds) - tgrad))^2 and sum ksqrt tgrad^2 in one stencil pass (``tcfd_h1_sums``);
    backward with respect to preds = the adjoint stencil (``tcfd_h1_sums_bwd``)."""

    @staticmethod
    def forward(ctx, preds, tgrad, ksqrt, kmode, h):
        pc, tc = preds.detach().contiguous(), tgrad.detach().contiguous()
        kc = ksqrt.detach().contiguous() if kmode else None
        N, C, n1, n2 = pc.shape
        lib = _lib.load()
        s1 = torch.empty(N, dtype=torch.float64, device=pc.device)
        s2 = torch.empty(N, dtype=torch.float64, device=pc.device)
        ws = torch.empty(lib.tcfd_h1_sums_workspace_bytes(N, C, n1, n2), dtype=torch.uint8, device=pc.device)
        with torch.cuda.device(pc.device):
            _lib.check(lib.tcfd_h1_sums(pc.data_ptr(), tc.data_ptr(), kc.data_ptr() if kmode else None, kmode, s1.data_ptr(),
                                        s2.data_ptr(), N, C, n1, n2, float(h), _code(pc.dtype), ws.data_ptr(), ws.numel(),
                                        _stream_ptr(pc.device)), "tcfd_h1_sums")
        ctx.save_for_backward(preds, tc, kc if kmode else pc.new_empty(0))
        ctx.cfg = (kmode, h)
        ctx.mark_non_differentiable(s2)
        return s1, s2

    @staticmethod
    def backward(ctx, g1, g2):
        preds, tc, kc = ctx.saved_tensors
        kmode, h = ctx.cfg
        if torch.is_grad_enabled():
            with torch.enable_grad():
                pin = preds if preds.requires_grad else preds.detach().requires_grad_(True)
                s1, _ = _h1_sums_ops(pin, tc, kc if kmode else None, h)
                (gp,) = torch.autograd.grad((s1 * g1).sum(), pin, create_graph=True)
            return gp, None, None, None, None
        pc = preds.detach().contiguous()
        N, C, n1, n2 = pc.shape
        cot = g1.detach().to(torch.float64).contiguous()
        grad = torch.empty_like(pc)
        with torch.cuda.device(pc.device):
            _lib.check(_lib.load().tcfd_h1_sums_bwd(pc.data_ptr(), tc.data_ptr(), kc.data_ptr() if kmode else None, kmode,
                                                    cot.data_ptr(), grad.data_ptr(), N, C, n1, n2, float(h), _code(pc.dtype),
                                                    _stream_ptr(pc.device)), "tcfd_h1_sums_bwd")
        return grad, None, None, None, None


class L2Loss2d(nn.Module):
    """fno/losses.py:50-137: per sample beta * weights * sum (p - t)^2 / (sum t^2 + eps), plus -- with ``targets_grad`` -- the H^1
    term gamma * mean (sqrt(K) (central_diff(p) - targets_grad))^2 / (2 mean(sqrt(K) targets_grad^2) + eps) (the reference
    replaces K by its square root before BOTH uses), then ``metric_reduction`` "L1" (sqrt, mean), "L2" (mean, sqrt) or "Linf".
    The two sums of the main term are one pass (``tcfd_lp_sums``), the H^1 sums one stencil pass (``tcfd_h1_sums``), for
    ``channel_last=False``, no ``weights`` tensor, ``noise == 0`` and K = None, a number / 0-dim tensor or (N, 1, n, n);
    everything else (and targets that need a gradient) runs the reference's tensor operations."""

    def __init__(self, regularizer=False, h=1 / 512, beta=1.0, gamma=1e-1, metric_reduction="L1", noise=0.0, eps=1e-3,
                 weighted=False, channel_last=False, debug=False):
        super().__init__()
        self.noise, self.regularizer, self.h, self.beta, self.gamma, self.eps = noise, regularizer, h, beta, gamma, eps
        self.metric_reduction, self.weighted, self.channel_last, self.debug = metric_reduction, weighted, channel_last, debug

    @staticmethod
    def _noise(targets: torch.Tensor, noise=0.0):
        assert 0 <= noise <= 0.2
        with torch.no_grad():
            targets = targets * (1.0 + noise * torch.rand_like(targets))
        return targets

    def _metric(self, loss):
        if self.metric_reduction == "L2":
            return loss.mean().sqrt()
        if self.metric_reduction == "L1":
            return loss.sqrt().mean()
        if self.metric_reduction == "Linf":
            return loss.sqrt().max()
        return loss

    def _tensor_ops(self, preds, targets, targets_grad, K, weights):
        K = torch.tensor(1) if K is None else K ** (0.5)
        if self.noise > 0:
            targets = self._noise(targets, self.noise)
        target_norm = targets.pow(2).sum(dim=(1, 2, 3)) + self.eps
        if weights is None and self.weighted:
            inv_l2 = 1 / target_norm.sqrt()
            weights = inv_l2 / inv_l2.mean()
        elif not self.weighted:
            weights = 1
        loss = self.beta * weights * ((preds - targets).pow(2)).sum(dim=(1, 2, 3)) / target_norm
        if targets_grad is not None:
            prime_norm = 2 * (K * targets_grad.pow(2)).mean(dim=(1, 2, 3)) + self.eps
            if self.gamma > 0:
                pg = torch.cat(central_diff(preds, channel_last=self.channel_last), dim=1)
                loss = loss + self.gamma * (K * (pg - targets_grad)).pow(2).mean(dim=(1, 2, 3)) / prime_norm
        return self._metric(loss)

    def _kmode(self, K, preds):
        if K is None:
            return 0, None
        if isinstance(K, (int, float)):
            return 1, torch.full((1,), float(K) ** 0.5, dtype=preds.dtype, device=preds.device)
        if torch.is_tensor(K) and K.ndim == 0 and not K.requires_grad:
            return 1, (K.to(device=preds.device, dtype=preds.dtype) ** 0.5).reshape(1)
        if (torch.is_tensor(K) and K.ndim == 4 and tuple(K.shape) == (preds.shape[0], 1) + tuple(preds.shape[2:])
                and K.dtype == preds.dtype and K.is_cuda and not K.requires_grad):
            return 2, K ** 0.5
        return -1, None

    def forward(self, preds, targets, targets_grad=None, K=None, weights=None):
        _need_hip(preds, targets, targets_grad)
        kmode, ksqrt = self._kmode(K, preds) if preds.ndim == 4 else (-1, None)
        fused = (kmode >= 0 and not self.channel_last and weights is None and self.noise == 0 and _lp_kernel_ok(preds, targets, 2, 1, preds.shape[0])
                 and not targets.requires_grad
                 and (targets_grad is None or (targets_grad.dtype == preds.dtype and not targets_grad.requires_grad
                                               and tuple(targets_grad.shape) == (preds.shape[0], 2 * preds.shape[1]) + tuple(preds.shape[2:]))))
        if not fused:
            return self._tensor_ops(preds, targets, targets_grad, K, weights)
        N = preds.shape[0]
        sd, sy = hip_lp_sums(preds, targets, N, preds.numel() // N, 1, 2, True)
        target_norm = sy[:, 0] + self.eps
        if self.weighted:
            inv_l2 = 1 / target_norm.sqrt()
            w = inv_l2 / inv_l2.mean()
        else:
            w = 1
        loss = self.beta * w * sd[:, 0] / target_norm
        if targets_grad is not None and self.gamma > 0:
            s1, s2 = _H1SumsFn.apply(preds, targets_grad, ksqrt, kmode, 1 / preds.shape[-1])
            count = targets_grad.numel() // N
            loss = loss + self.gamma * (s1 / count) / (2 * (s2 / count) + self.eps)
        return self._metric(loss.to(preds.dtype))


class BochnerNorm(SobolevLoss):
    """The space-time norm (int ||u||_p^2 dt)^(1/2), fno/losses.py:318-364: per (b, t) the p-norm over space (/ n when mesh
    weighted), then sqrt(mean_t) (``time_average`` without ``dt``) or sqrt(sum_t * dt), then the batch mean (``reduction``) or sum.
    The reference's constructor hands ``time_last=`` to a parent without that parameter and cannot be called; this one takes
    the same arguments and works.  With neither ``time_average`` nor ``dt`` the reference's forward dies on an unbound name:
    ``ValueError`` here.  The spatial sums are one pass over u in either layout (``tcfd_lp_sums``)."""

    def __init__(self, n_grid=256, dt: float = None, p: int = 2, relative=True, mesh_weighted=True, reduction=True,
                 time_average=False, time_last=False):
        super().__init__(n_grid=n_grid, relative=relative, inp_time_last=time_last, reduction=reduction,
                         mesh_weighted=mesh_weighted, time_average=time_average)
        self.time_last, self.dt, self.p = time_last, dt, p

    def forward(self, u):
        if not self.time_average and self.dt is None:
            raise ValueError("BochnerNorm needs time_average=True or a time step dt")
        _need_hip(u)
        n = self.n_grid
        if u.ndim == 3:
            u = u.unsqueeze(0)
        b = u.shape[0]
        if self.time_last:
            outer, reduce, inner = b, u.shape[1] * u.shape[2], u.shape[3]
        else:
            outer, reduce, inner = b * u.shape[1], u.shape[2] * u.shape[3], 1
        if _lp_kernel_ok(u, None, self.p, inner, outer):
            sd, _ = hip_lp_sums(u, None, outer, reduce, inner, self.p, False)
            norm_space = (sd.reshape(b, -1) ** (1.0 / self.p)).to(u.dtype)
        else:
            ut = u if self.time_last else u.permute(0, 2, 3, 1)
            norm_space = ut.abs().pow(self.p).sum(dim=(1, 2)) ** (1 / self.p)
        norm_space = norm_space / n if self.mesh_weighted else norm_space
        if self.time_average and self.dt is None:
            norm = ((norm_space**2).mean(dim=-1)).sqrt()
        else:
            norm = ((norm_space**2).sum(dim=-1) * self.dt).sqrt()
        return norm.mean() if self.reduction else norm.sum()


_RES_GRIDS = (16, 32, 64, 128, 256, 512, 1024, 96, 192, 384, 768, 80, 160, 320, 640)
_FFT_SCALE = {"backward": lambda n3: 1.0, None: lambda n3: 1.0, "ortho": lambda n3: 1.0 / math.sqrt(n3), "forward": lambda n3: 1.0 / n3}


class _ResidualFn(torch.autograd.Function):
    """The fused residual loss as one autograd node: forward = the seven launches of ``tcfd_residual_loss`` (the squared row norms
    kept), backward = ``tcfd_residual_loss_backward`` (the planes are recomputed, nothing else crosses the training step)."""

    @staticmethod
    def forward(ctx, w, f, module, plan, tabs, scale):
        wc = w.detach()
        fc = f.detach() if f is not None else None
        out, rows = module._launch_forward(plan, wc, fc, tabs, scale)
        ctx.save_for_backward(w, f if f is not None else w.new_empty(0), rows)
        ctx.cfg = (module, plan, tabs, scale, f is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        w, f, rows = ctx.saved_tensors
        module, plan, tabs, scale, has_f = ctx.cfg
        f = f if has_f else None
        need_w, need_f = ctx.needs_input_grad[0], has_f and ctx.needs_input_grad[1]
        if torch.is_grad_enabled():
            # create_graph=True: the raw-pointer launches would return constants and silently drop every second-order term.
            # Differentiate the composed loss (Rfft2 / Irfft2 + tensor operations, differentiable any number of times) instead.
            with torch.enable_grad():
                win = w if w.requires_grad else w.detach().requires_grad_(True)
                fin = (f if f.requires_grad else f.detach().requires_grad_(True)) if need_f else f
                loss = module._composed(win, None, fin)
                gs = torch.autograd.grad(loss, [win] + ([fin] if need_f else []), gout.to(loss.dtype), create_graph=True)
            return (gs[0] if need_w else None), (gs[1] if need_f else None), None, None, None, None
        wc = w.detach()
        lib = _lib.load()
        bsz, n, _, nt = wc.shape
        gw = torch.empty_like(wc) if need_w else None
        gf = torch.empty_like(wc) if need_f else None
        g = gout.detach().to(wc.dtype).contiguous()
        ws = torch.empty(lib.tcfd_residual_workspace_bytes(plan, bsz, nt, 1), dtype=torch.uint8, device=wc.device)
        m2pi, lap, ckt, twt = tabs
        with torch.cuda.device(wc.device):
            _lib.check(lib.tcfd_residual_loss_backward(
                plan, wc.data_ptr(), f.data_ptr() if has_f else None, m2pi.data_ptr(), lap.data_ptr(), ckt.data_ptr(), twt.data_ptr(),
                float(module.visc), scale, rows.data_ptr(), g.data_ptr(), bsz, nt, gw.data_ptr() if need_w else None,
                gf.data_ptr() if need_f else None, ws.data_ptr(), ws.numel(), _stream_ptr(wc.device)), "tcfd_residual_loss_backward")
        return gw, gf, None, None, None, None


class ResidualLoss(nn.Module):
    """The physics-informed residual of the vorticity equation over a predicted block, fno/losses.py:367-467: with every transform
    an fftn / ifftn over (x, y, t) of the time-last (b, n, n, T) tensors,

        res = Re( 2 pi i kt w^ + fftn(psi_y w_x - psi_x w_y) - visc lap w^ - f^ ),   psi^ = -w^ / lap  (or fftn(psi)),

    loss = mean over (b, kx) of the 2-norm over (ky, kt) of res, / n.  ``lap`` carries 1 on the whole line kx = ky = 0, so the
    mean mode keeps -visc w^(0, 0, kt).  The tables ``kx, ky, kt, lap`` are plain attributes of shape (batch_size, n, n, n_t)
    in the default dtype of the moment of construction (not buffers, not in ``state_dict``) and keep that rounding: a
    float32-built module on float64 data uses float32-rounded tables, as torch's promotion does in the reference.

    The multipliers 2 pi i kx, 2 pi i ky break Hermitian symmetry on the Nyquist row / column, so the four physical fields are
    complex; their imaginary parts move the loss by 4e-7 .. 4e-5 and are kept.

    On the grids of the loss kernels (2^k in [16, 1024], 3 * 2^k in [96, 768], 5 * 2^k in [80, 640]) with T <= 128 and ``psi``
    not given, the value is seven launches on the tensors in place and the gradient with respect to ``w`` and ``f`` thirteen
    (csrc/tcfd_residual.hip); the time transforms that cancel are never run and no 3-D spectrum is formed.  Everything else --
    ``psi`` given, other shapes, ``TCFD_RESIDUAL_FUSED=0``, a graph of the gradient itself -- is ``_composed``: the package's
    real 2-D transforms (``autograd.Rfft2`` / ``Irfft2``), the Nyquist parts in closed form, a dense time DFT."""

    def __init__(self, batch_size=1, alpha=1e-1, visc=1e-3, n_grid=64, n_t=40, delta_t=1e-2, norm="ortho"):
        super().__init__()
        if norm not in _FFT_SCALE:
            raise ValueError(f"unknown fft norm {norm!r}")
        self.batch_size, self.alpha, self.visc, self.n_grid = batch_size, alpha, visc, n_grid
        self.delta_t, self.n_t, self.norm = delta_t, n_t, norm
        self._set_spectral_laplacian_spacetime()

    def _set_spectral_laplacian_spacetime(self):
        n, n_t = self.n_grid, self.n_t
        k = torch.fft.fftfreq(n, d=1 / n)
        kt = torch.fft.fftfreq(n_t, d=self.delta_t)
        kx, ky, kt = torch.meshgrid([k, k, kt], indexing="ij")
        lap = -4 * (torch.pi**2) * (kx**2 + ky**2)
        lap[0, 0] = 1
        self.kx, self.ky, self.kt, self.lap = [z.unsqueeze(0).expand(self.batch_size, n, n, n_t) for z in (kx, ky, kt, lap)]
        self._tab_cache = {}

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_tab_cache"] = {}          # device-side tables are rebuilt on demand
        return state

    def _tables(self, device, dtype):
        """(m2pi[n], lap[n, n], ckt[T], twt[T] complex) on the device in the data's precision, from the module's own tables: the
        products 2 pi k are formed in the TABLES' dtype, as the reference forms them.  Cached per (device, dtype)."""
        key = (torch.device(device), dtype, self.kx.data_ptr(), self.lap.data_ptr(), self.kt.data_ptr())
        cached = self._tab_cache.get(key)
        if cached is None:
            m2pi = (2 * torch.pi * self.kx[0, :, 0, 0].cpu())
            ckt = (2 * torch.pi * self.kt[0, 0, 0, :].cpu())
            lap = self.lap[0, :, :, 0].cpu()
            ang = -2 * torch.pi * torch.arange(self.n_t, dtype=torch.float64) / self.n_t
            twt = torch.complex(torch.cos(ang), torch.sin(ang)).to(torch.complex128 if dtype == torch.float64 else torch.complex64)
            cached = tuple(t.to(device=device, dtype=t.dtype if t.is_complex() else dtype).contiguous() for t in (m2pi, lap, ckt, twt))
            self._tab_cache[key] = cached
        return cached

    def _scale(self, bsz):
        n = self.n_grid
        return _FFT_SCALE[self.norm](n * n * self.n_t) / (bsz * n * n)

    def _launch_forward(self, plan, wc, fc, tabs, scale):
        lib = _lib.load()
        bsz, n, _, nt = wc.shape
        out = torch.empty((), dtype=wc.dtype, device=wc.device)
        rows = torch.empty(bsz * n, dtype=torch.float64, device=wc.device)
        ws = torch.empty(lib.tcfd_residual_workspace_bytes(plan, bsz, nt, 0), dtype=torch.uint8, device=wc.device)
        m2pi, lap, ckt, twt = tabs
        with torch.cuda.device(wc.device):
            _lib.check(lib.tcfd_residual_loss(plan, wc.data_ptr(), fc.data_ptr() if fc is not None else None, m2pi.data_ptr(),
                                              lap.data_ptr(), ckt.data_ptr(), twt.data_ptr(), float(self.visc), scale, bsz, nt,
                                              out.data_ptr(), rows.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(wc.device)),
                       "tcfd_residual_loss")
        return out, rows

    def _fused(self, w, f):
        """The loss on the fused kernels, or None outside their cover."""
        if os.environ.get("TCFD_RESIDUAL_FUSED", "1") == "0" or w.dtype not in (torch.float32, torch.float64):
            return None
        bsz, n, _, nt = w.shape
        if n not in _RES_GRIDS or bsz == 0 or bsz > 65535:
            return None
        lib = _lib.load()
        code = _code(w.dtype)
        pkey = (n, code, w.device)
        plan = _LOSS_PLANS.get(pkey)
        if plan is None:
            handle = ctypes.c_void_p()
            with torch.cuda.device(w.device):
                _lib.check(lib.tcfd_loss_plan_create(ctypes.byref(handle), n, code), "tcfd_loss_plan_create")
            plan = _LOSS_PLANS[pkey] = handle
        if not lib.tcfd_residual_loss_supported(plan, nt):
            return None
        tabs = self._tables(w.device, w.dtype)
        wc = w.contiguous()
        fc = f.contiguous() if f is not None else None
        scale = self._scale(bsz)
        if torch.is_grad_enabled() and (w.requires_grad or (f is not None and f.requires_grad)):
            return _ResidualFn.apply(wc, fc, self, plan, tabs, scale)
        return self._launch_forward(plan, wc, fc, tabs, scale)[0]

    def forward(self, w, psi=None, f=None):
        if w.ndim != 4 or w.shape[1] != w.shape[2]:
            raise ValueError(f"expected (b, n, n, T), got {tuple(w.shape)}")
        bsz, n, _, nt = w.shape
        if n != self.n_grid:
            raise ValueError(f"grid {n} != n_grid {self.n_grid}")
        if nt != self.n_t:
            raise ValueError(f"{nt} time steps != n_t {self.n_t}")
        if bsz != self.batch_size and self.batch_size != 1:
            raise ValueError(f"batch {bsz} != batch_size {self.batch_size} (the tables broadcast only from batch_size 1)")
        for name, z in (("psi", psi), ("f", f)):
            if z is not None and z.shape != w.shape:
                raise ValueError(f"{name} {tuple(z.shape)} != w {tuple(w.shape)}")
        _need_hip(w, psi, f)
        # torch's promotion in the reference: data meets the tables' dtype in every product
        cdt = torch.promote_types(w.dtype, self.kx.dtype)
        w, psi, f = (z.to(cdt) if z is not None else None for z in (w, psi, f))
        if psi is None:
            fused = self._fused(w, f)
            if fused is not None:
                return fused
        return self._composed(w, psi, f)

    def _composed(self, w, psi=None, f=None):
        """The same loss from the package's differentiable real transforms and tensor operations.  Each multiplied field is split:
        its Hermitian part (the Nyquist row / column of the multiplier zeroed) comes back real through ``Irfft2``; the rest lives on
        that one row / column and is purely imaginary in physical space, (-1)^x (m_N / n) sum_x' (-1)^x' h(x', y) for an
        x-derivative of h (likewise in y).  The product is complex; Re fftn(A + i B) = Re A^ - Im B^ is evaluated on the half
        spectra of A and B at k and at -k, after a dense real time DFT."""
        from .autograd import Irfft2 as _Irfft2Fn
        from .equations import fft_plan

        bsz, n, _, nt = w.shape
        if n % 2:
            raise ValueError("the composed residual loss takes even grids")
        dev, rdt = w.device, w.dtype
        cdtype = torch.complex64 if rdt == torch.float32 else torch.complex128
        plan = fft_plan(n, cdtype, dev, 1.0)
        m2pi, lap, ckt, _ = self._tables(dev, rdt)
        m, h = n // 2 + 1, n // 2
        mx = m2pi[:, None].clone()
        my = m2pi[None, :m].clone()
        c_ny = m2pi[h] / n
        mx[h] = 0
        my[:, h] = 0
        laph = lap[:, :m]
        sign = 1 - 2 * (torch.arange(n, device=dev) % 2).to(rdt)            # (-1)^j

        R = lambda z: _Rfft2Fn.apply(z.contiguous(), plan)
        I = lambda z: _Irfft2Fn.apply(z.contiguous(), plan)
        tf = lambda z: z.permute(0, 3, 1, 2)                                # (b, n, n, T) -> (b, T, n, n)
        wt = tf(w)
        wh = R(wt)
        if psi is not None:
            pt = tf(psi)
            ph = R(pt)
        else:
            ph = -wh / laph
            pt = I(ph)
        alt_x = lambda z: sign[:, None] * c_ny * (z * sign[:, None]).sum(dim=-2, keepdim=True)     # Im of an x-derivative
        alt_y = lambda z: sign[None, :] * c_ny * (z * sign[None, :]).sum(dim=-1, keepdim=True)     # Im of a y-derivative
        q_r, q_i = I(1j * my * ph), alt_y(pt)
        v_r, v_i = I(-1j * mx * ph), -alt_x(pt)
        wx_r, wx_i = I(1j * mx * wh), alt_x(wt)
        wy_r, wy_i = I(1j * my * wh), alt_y(wt)
        prod_r = q_r * wx_r - q_i * wx_i + v_r * wy_r - v_i * wy_i
        prod_i = q_r * wx_i + q_i * wx_r + v_r * wy_i + v_i * wy_r
        hh = R(prod_r - tf(f) if f is not None else prod_r) - self.visc * (laph * wh)
        bh = R(prod_i)
        ang = 2 * torch.pi * torch.outer(torch.arange(nt, dtype=torch.float64), torch.arange(nt, dtype=torch.float64)) / nt
        cm, sm = torch.cos(ang).to(dev, rdt), torch.sin(ang).to(dev, rdt)
        dft = lambda mat, z: torch.einsum("kt,btxy->bkxy", mat, z)
        ck = ckt[None, :, None, None]
        hr, hi, br, bi, wr, wi = hh.real, hh.imag, bh.real, bh.imag, wh.real, wh.imag
        res_p = dft(cm, hr - bi) + dft(sm, hi + br) - ck * (dft(cm, wi) - dft(sm, wr))
        res_m = dft(cm, hr + bi) + dft(sm, br - hi) + ck * (dft(cm, wi) + dft(sm, wr))
        flip = (-torch.arange(n, device=dev)) % n
        res = torch.cat([res_p, res_m[:, :, flip, 1:h]], dim=3)            # (b, kt, kx, all ky)
        rows = torch.linalg.norm(res, dim=(1, 3))                           # (b, kx)
        return rows.sum() * self._scale(bsz)
