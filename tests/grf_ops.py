"""Plain-torch restatement of what ``tcfd_grf_spectrum`` computes, for the tests (CPU or any device, any dtype).

With V = sqrt_eig * (noise[:, 0] + i noise[:, 1]) on the n0 mesh, H(k) = (V(k) + conj V(-k mod n0)) / 2 and st = n0 / n:

    rfft2(Re(ifft2(V))[..., ::st, ::st])[kx, ky] = (n / n0)^2 * sum_{a, b < st} H(kx + a n, ky + b n)

and ||Re(ifft2(V)) / n0||_F = sqrt(sum_k |H(k)|^2) / n0^2 (Parseval).  tests/test_grf_host.py checks this file against
the reference's recorded samples, which makes it an oracle at the sizes no golden covers.
"""
import torch
import torch.nn.functional as F


def seeded_noise(seed: int, bsz: int, mesh: int, dtype=torch.float64) -> torch.Tensor:
    """(bsz, 2, mesh, mesh) from one CPU stream seeded with ``seed``."""
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randn(bsz, 2, mesh, mesh, generator=gen, dtype=dtype)


def smoothed(noise: torch.Tensor, n: int) -> torch.Tensor:
    return F.interpolate(noise, size=(n, n), mode="bilinear")


def hermitian_part(noise: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    n0 = table.shape[-1]
    v = table * torch.complex(noise[:, 0], noise[:, 1])
    idx = (-torch.arange(n0, device=noise.device)) % n0
    return 0.5 * (v + v[:, idx][:, :, idx].conj())


def fold_spectrum(noise: torch.Tensor, table: torch.Tensor, n: int, normalize: bool = False) -> torch.Tensor:
    """(B, 2, n0, n0) noise, (n0, n0) table -> (B, n, n/2 + 1) half spectrum of the sample sub-sampled to n."""
    bsz, n0 = noise.shape[0], table.shape[-1]
    st = n0 // n
    assert st * n == n0
    h = hermitian_part(noise, table.to(noise.dtype))
    hat = h.reshape(bsz, st, n, st, n).sum(dim=(1, 3)) * (n / n0) ** 2
    if normalize:
        norm = torch.sqrt((h.abs() ** 2).sum(dim=(-2, -1))) / n0**2
        hat = hat / norm[:, None, None]
    return hat[..., : n // 2 + 1]


def field(hat: torch.Tensor) -> torch.Tensor:
    n = hat.shape[-2]
    return torch.fft.irfft2(hat, s=(n, n))
