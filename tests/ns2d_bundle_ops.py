"""Helpers of the tangent-bundle tests (tests/test_ns2d_bundle_host.py, tests/test_ns2d_bundle_gpu.py): the forward-mode
reference of a bundle and seeded bundles of smooth perturbations."""
import functools

import torch

import ns2d_ops

CPLX = {"f64": torch.complex128, "f32": torch.complex64}


def oracle_bundle(fn, w, dW):
    """``(fn(w), [d fn(w) . dW[k]])`` for a bundle ``dW`` = (K,) + w.shape by ONE forward_ad evaluation: the state repeated K
    times along the batch, tangent k riding on copy k.  ``fn`` maps (batch, n, m) to (batch, n, m), sample by sample."""
    K = dW.shape[0]
    lead = w.shape[:-2]
    wb = w.reshape((-1,) + w.shape[-2:])
    rep = wb.repeat(K, 1, 1)
    primal, tangent = ns2d_ops.jvp(fn, rep, dW.reshape(rep.shape))
    return primal[: wb.shape[0]].reshape(lead + w.shape[-2:]), tangent.reshape(dW.shape)


def _smooth_fields(n, count, k0, seed):
    """`count` seeded real fields with a Gaussian spectrum of width k0 and rms 5, as fp64 half spectra."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64)
    env = torch.exp(-(k[:, None] ** 2 + k[None, : n // 2 + 1] ** 2) / (2.0 * k0 * k0))
    w = torch.fft.irfft2(torch.fft.rfft2(torch.randn(count, n, n, generator=gen, dtype=torch.float64)) * env, s=(n, n))
    return torch.fft.rfft2(5.0 * w / w.std())


@functools.lru_cache(maxsize=None)
def inputs(n, tag, B, K):
    """(w0, dW) on the CPU in the precision of `tag`: B smooth random vorticity fields and K x B distinct smooth perturbations
    of different widths and amplitudes (up to three distinct states, repeated with other amplitudes for larger batches)."""
    k0 = min(4.0, n / 6.0)
    nb = min(B, 3)
    w0 = _smooth_fields(n, nb, k0, 1000 + n)
    reps = (B + nb - 1) // nb
    scale = (1 + 0.1 * torch.arange(B, dtype=torch.float64))[:, None, None]
    w0 = w0.repeat(reps, 1, 1)[:B] * scale
    dW = torch.stack([_smooth_fields(n, nb, (1.0 + 0.5 * (k % 3)) * k0, 3000 + 17 * k + n).repeat(reps, 1, 1)[:B] * scale.flip(0)
                      * (0.5 + 0.25 * k) for k in range(K)])
    return w0.to(CPLX[tag]).contiguous(), dW.to(CPLX[tag]).contiguous()
