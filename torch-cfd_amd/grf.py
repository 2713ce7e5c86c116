"""Gaussian random fields with covariance ``(-Laplacian + tau^2)^(-alpha)`` on the periodic unit square: the initial
condition of the FNO-paper data set.

Drop-in for ``GRF2d`` of the reference (fno/data_gen/grf.py:13-124).  The reference draws complex white noise ``c`` on an
n x n mesh and returns ``Re(ifft2(sqrt_eig * c))``; its driver (fno/data_gen/data_gen_fno.py:195-205) samples at 2048^2 for a
"replicable init", keeps every (2048 / n)-th point (``F.interpolate(mode="nearest")`` with n | 2048 is exactly that stride)
and calls ``rfft2``.  Here the half spectrum of that whole chain comes from ONE pass of a HIP kernel over the noise
(``tcfd_grf_spectrum``, csrc/tcfd_grf.hip: Hermitian part of ``sqrt_eig * c``, aliases folded, optional normalisation by
Parseval), and ``sample`` is the HIP ``irfft2`` of it.

The noise is the reference's CPU stream (its ``device="cpu"`` path: one generator seeded with ``random_state``,
``randn(bsz, 2, n, n)``), uploaded in chunks of at most ``NOISE_BYTES_CAP`` bytes.  The noise of the reference's CUDA generator is
not reproducible here.  ``sqrt_eig`` tables are built on the CPU with the reference's expression (bit-equal) and kept PER
SIZE: the reference overwrites ``self.sqrt_eig`` when it samples at another n and then fails at the original one.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .equations import _COMPLEX_OF, fft_plan

NOISE_BYTES_CAP = 1 << 30   # staged noise, host and device each: 16 samples of 2048^2 float64


def noise_chunks(count: int, n0: int, itemsize: int, cap_bytes: int = NOISE_BYTES_CAP) -> List[Tuple[int, int]]:
    """``(start, count)`` pieces of a batch of ``count`` noise samples (2 planes of n0 x n0 reals of ``itemsize`` bytes each),
    in order, each piece at most ``cap_bytes`` -- or one sample where a single one is already larger."""
    per_sample = 2 * n0 * n0 * itemsize
    step = max(1, cap_bytes // per_sample)
    return [(s, min(step, count - s)) for s in range(0, count, step)]


def sqrt_eig_table(n: int, alpha: float, tau: float, dim: int = 2, sigma: Optional[float] = None) -> torch.Tensor:
    """(n, n) square roots of the covariance eigenvalues, on the CPU in the torch default dtype: the expression of
    ``GRF2d._initialize`` (grf.py:54-77) operation for operation, so the table equals the reference's bit for bit."""
    sigma = tau ** (0.5 * (2 * alpha - dim)) if sigma is None else sigma
    h = 1 / n
    k = torch.fft.fftfreq(n, d=h)
    kx, ky = torch.meshgrid(k, k, indexing="ij")
    table = (n**dim) * math.sqrt(2.0) * sigma * ((4 * (math.pi**2) * (kx**2 + ky**2) + tau**2) ** (-alpha / 2.0))
    table[0, 0] = 0.0
    return table


class GRF2d(nn.Module):
    """Gaussian random field on [0, 1]^2 with mean 0 and covariance ``(-Laplacian + tau^2)^(-alpha)``; constructor,
    attributes, ``sample`` and ``forward`` as the reference's class.  ``sample_hat`` is new: the half spectrum (the layout
    of ``rfft2``) of one sample per seed, optionally drawn at ``n0`` and sub-sampled to ``n`` (the driver's replicable init).

    HIP only: sampling with ``device="cpu"`` raises ``TcfdError``."""

    def __init__(self, *, dim=2, n=128, alpha=2, tau=3, device="cuda", dtype=torch.float, normalize=False, smoothing=False,
                 **kwargs):
        super().__init__()
        if dim != 2:
            raise NotImplementedError("GRF2d: dim = 2 only, as the reference's sample()")
        self.dim = dim
        self.n = n
        self.device = device
        self.dtype = dtype
        self.normalize = normalize
        self.alpha = alpha
        self.tau = tau
        self.smoothing = smoothing
        self.max_mesh_size = 2048
        self._tables: Dict[int, torch.Tensor] = {}          # n -> CPU table
        self._device_tables: Dict[tuple, torch.Tensor] = {}  # (n, real dtype, device) -> uploaded table
        self._table(n)

    # -- tables
    def _table(self, n: int) -> torch.Tensor:
        t = self._tables.get(n)
        if t is None:
            t = self._tables[n] = sqrt_eig_table(n, self.alpha, self.tau, self.dim)
        return t

    @property
    def sqrt_eig(self) -> torch.Tensor:
        """The table of the module's own size ``n`` (on the CPU; the kernels read an uploaded copy)."""
        return self._table(self.n)

    def _device_table(self, n: int, real: torch.dtype, device: torch.device) -> torch.Tensor:
        key = (n, real, device)
        t = self._device_tables.get(key)
        if t is None:
            t = self._device_tables[key] = self._table(n).to(device=device, dtype=real).contiguous()
        return t

    def _compute_dtype(self, n: int) -> torch.dtype:
        # the reference multiplies the table (torch default dtype) by the complex noise (self.dtype): torch promotes
        return torch.promote_types(self._table(n).dtype, self.dtype)

    def _hip_device(self, device=None) -> torch.device:
        device = torch.device(self.device if device is None else device)
        if device.type != "cuda":
            raise _lib.TcfdError(f"GRF2d samples on HIP devices only (no CPU fallback); got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    # -- noise
    def _draw(self, gens: Sequence[torch.Generator], count_each: int, mesh: int) -> torch.Tensor:
        """(len(gens) * count_each, 2, mesh, mesh) CPU noise, ``count_each`` consecutive samples from every generator."""
        out = torch.empty((len(gens) * count_each, 2, mesh, mesh), dtype=self.dtype)

        def draw(i):
            torch.randn((count_each, 2, mesh, mesh), generator=gens[i], out=out[i * count_each:(i + 1) * count_each])

        if len(gens) < 4:
            for i in range(len(gens)):
                draw(i)
        else:   # independent generators: a few threads (the draw releases the GIL), as initial_conditions._seeded_noise
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=min(16, len(gens))) as pool:
                list(pool.map(draw, range(len(gens))))
        return out

    def _spectrum(self, noise: torch.Tensor, n: int, out: torch.Tensor) -> None:
        """Kernel call: noise (c, 2, n0, n0) on the device -> out (c, n, n/2 + 1)."""
        lib = _lib.load()
        count, _, n0, _ = noise.shape
        real = out.real.dtype
        noise = noise.to(real).contiguous()
        table = self._device_table(n0, real, noise.device)
        need = lib.tcfd_grf_spectrum_workspace_bytes(count, n, int(bool(self.normalize)))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=noise.device)
        with torch.cuda.device(noise.device):
            rc = lib.tcfd_grf_spectrum(noise.data_ptr(), table.data_ptr(), out.data_ptr(), count, n0, n,
                                       _lib.TCFD_C128 if real == torch.float64 else _lib.TCFD_C64, int(bool(self.normalize)),
                                       ws.data_ptr(), need, ctypes.c_void_p(torch.cuda.current_stream(noise.device).cuda_stream))
        _lib.check(rc, "tcfd_grf_spectrum")

    def _sample_hat(self, seeds: Sequence[int], count_each: int, n: int, n0: int, device) -> torch.Tensor:
        """Spectra of ``count_each`` consecutive samples of every seed's stream (sample: one seed, bsz samples; sample_hat:
        one sample per seed)."""
        if n0 % n or n % 2:
            raise NotImplementedError(f"GRF2d: an even n that divides n0 only (nearest sub-sampling is a stride then); "
                                      f"got n = {n}, n0 = {n0}")
        device = self._hip_device(device)
        # smoothing (grf.py:90-97): the noise is drawn at max_mesh_size and interpolated to the sampling mesh
        mesh = self.max_mesh_size if self.smoothing else n0
        real = self._compute_dtype(n0)
        total = len(seeds) * count_each
        out = torch.empty((total, n, n // 2 + 1), dtype=_COMPLEX_OF[real], device=device)
        itemsize = torch.empty(0, dtype=real).element_size()
        if count_each != 1:
            # one stream cut into pieces: the normal fill works on runs of 16 values, so the pieces continue the stream of the
            # single randn(bsz, ...) call only when a sample is a whole number of runs
            assert len(seeds) == 1
            gen = torch.Generator().manual_seed(int(seeds[0]))
            pieces = noise_chunks(total, mesh, itemsize) if (2 * mesh * mesh) % 16 == 0 else [(0, total)]
            for start, count in pieces:
                self._stage(self._draw([gen], count, mesh), n, n0, out[start:start + count], device)
        else:
            for start, count in noise_chunks(total, mesh, itemsize):
                gens = [torch.Generator().manual_seed(int(s)) for s in seeds[start:start + count]]
                self._stage(self._draw(gens, 1, mesh), n, n0, out[start:start + count], device)
        return out

    def _stage(self, noise: torch.Tensor, n: int, n0: int, out: torch.Tensor, device) -> None:
        noise = noise.to(device)
        if self.smoothing:
            noise = F.interpolate(noise, size=(n0, n0), mode="bilinear")
        self._spectrum(noise, n, out)

    # -- public
    def sample_hat(self, seeds: Sequence[int], n: Optional[int] = None, n0: Optional[int] = None, device=None) -> torch.Tensor:
        """(len(seeds), n, n/2 + 1) half spectra, sample i being ``rfft2`` of the reference's
        ``sample(1, n0, random_state=seeds[i])`` sub-sampled to n.  ``n0`` defaults to ``n``; it must be a multiple of n."""
        n = self.n if n is None else n
        n0 = n if n0 is None else n0
        return self._sample_hat(list(seeds), 1, n, n0, device)

    def sample(self, bsz, n=None, random_state=0, device=None, **kwargs) -> torch.Tensor:
        """(bsz, n, n) fields from ONE stream seeded with ``random_state`` (grf.py:79-115)."""
        n = self.n if n is None else n
        hat = self._sample_hat([random_state], bsz, n, n, device)
        return fft_plan(n, hat.dtype, hat.device).irfft2(hat)

    def forward(self, x, **kwargs):
        """x: (bsz, C, n, n) -> a sample of its batch size and mesh on its device."""
        bsz, _, *mesh_size = x.size()
        return self.sample(bsz, n=max(mesh_size), device=x.device, **kwargs)
