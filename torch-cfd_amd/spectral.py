"""Host-side pieces of the k-space arithmetic that callers of the reference name directly.

Only two functions of torch_cfd/spectral.py are part of the operator API the
spectral path is used through: ``brick_wall_filter_2d`` (the 2/3-rule mask that
becomes a plan table, spectral.py:78-84) and ``vorticity_to_velocity``
(spectral.py:87-115, here one launch of ``k_velocity``).  Everything else the
reference composes per RK stage from small helpers (Laplacian, gradient, rot,
curl) is arithmetic inside the HIP kernels (csrc/tcfd_ns2d.hip: ``emit_planes``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .grids import Grid


def dealias_extents(n: int) -> Tuple[int, int, int]:
    """(low rows kept, high rows kept, columns kept) of the 2/3-rule brick wall on an n x (n//2+1) half spectrum.

    The reference builds the mask with Python slices ``[: int(2/3*n)//2]`` and ``[-int(2/3*n)//2 :]``
    (spectral.py:82-83).  Unary minus binds tighter than ``//``, so the upper block keeps
    ``ceil(k/2)`` rows while the lower one keeps ``floor(k/2)``, k = int(2/3*n): n = 128 keeps 42 low and
    43 high rows.  The golden tables (tests/golden/ns2d_tables.npz) pin this.
    """
    k = int(2 / 3 * n)
    cols = int(2 / 3 * (n // 2 + 1))
    return k // 2, -(-k // 2), cols


def brick_wall_filter_2d(grid: Grid) -> torch.Tensor:
    """0/1 mask (n, n//2+1) in the default dtype on the CPU, as the reference returns it."""
    n = grid.shape[0]
    low, high, cols = dealias_extents(n)
    i = torch.arange(n)
    j = torch.arange(n // 2 + 1)
    rows_kept = (i < low) | (i >= n - high)
    return (rows_kept[:, None] & (j < cols)[None, :]).to(torch.get_default_dtype())


def vorticity_to_velocity(grid: Grid, w_hat: torch.Tensor,
                          rfft_mesh: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """``((u_hat, v_hat), psi_hat)`` of a vorticity half spectrum ``(*, n, m)`` on a HIP device:
    psi = -w / lap (lap(0,0) := 1), u = 2 pi i ky psi, v = -2 pi i kx psi -- one launch of ``k_velocity``."""
    from .equations import _plan_for_mesh  # late: equations imports this module

    kx, ky = grid.rfft_mesh() if rfft_mesh is None else rfft_mesh
    if tuple(kx.shape[-2:]) != tuple(w_hat.shape[-2:]):
        raise ValueError(f"wavenumber mesh {tuple(kx.shape[-2:])} does not match the spectrum {tuple(w_hat.shape[-2:])}")
    return _plan_for_mesh(kx, ky, w_hat).velocity(w_hat)


# ----------------------------------------------------------------------------- k-space helpers callers name directly
# Plain tensor expressions on whatever device their arguments live on (torch_cfd/spectral.py:29-75).  The operator
# itself never calls them -- the same arithmetic is fused into the HIP kernels -- they are here so that scripts written
# against the reference (diagnostics, custom forcings, post-processing) keep working.
_TWO_PI_I = 2j * torch.pi


def fft_mesh_2d(n: int, diam: float, device=None):
    """Full (n, n) wavenumber mesh (cycles per unit length), ``indexing='ij'``."""
    k = torch.fft.fftfreq(n, d=diam / n)
    kx, ky = torch.meshgrid(k, k, indexing="ij")
    return kx.to(device), ky.to(device)


def spectral_laplacian_2d(fft_mesh, device=None) -> torch.Tensor:
    """Symbol of the Laplacian, ``-(2 pi)^2 |k|^2``, with the (0, 0) entry set to 1 so that it can be divided by."""
    kx, ky = fft_mesh
    lap = -((2 * torch.pi) ** 2) * (kx.abs() ** 2 + ky.abs() ** 2)
    lap[..., 0, 0] = 1
    return lap.to(device)


def spectral_grad_2d(f_hat: torch.Tensor, rfft_mesh):
    """(d/dx, d/dy) of a scalar half spectrum."""
    kx, ky = rfft_mesh
    return _TWO_PI_I * kx * f_hat, _TWO_PI_I * ky * f_hat


def spectral_rot_2d(psi_hat: torch.Tensor, rfft_mesh):
    """Velocity of a stream function: (d psi / dy, -d psi / dx)."""
    dx, dy = spectral_grad_2d(psi_hat, rfft_mesh)
    return dy, -dx


def spectral_curl_2d(vel_hat, rfft_mesh) -> torch.Tensor:
    """Scalar curl dv/dx - du/dy of a velocity pair of half spectra."""
    u_hat, v_hat = vel_hat
    kx, ky = rfft_mesh
    return _TWO_PI_I * (kx * v_hat - ky * u_hat)


def spectral_div_2d(vel_hat, rfft_mesh) -> torch.Tensor:
    """Divergence du/dx + dv/dy of a velocity pair of half spectra."""
    u_hat, v_hat = vel_hat
    kx, ky = rfft_mesh
    return _TWO_PI_I * (kx * u_hat + ky * v_hat)


def real_field_weights(n: int, m: int, dtype=torch.float64, device=None) -> torch.Tensor:
    """Column weights ``c`` of the real-field inner product on an ``(n, m)`` half spectrum (``m = n // 2 + 1``, torch's
    unnormalised ``rfft2``):  sum_x a(x) b(x) = sum_{ij} c_j Re(conj(a^_ij) b^_ij).  The ky = 0 column stands for itself,
    every interior column also for its mirror image (weight 2), and for even ``n`` the Nyquist column for itself again; the
    1 / n^2 of Parseval's identity is folded in."""
    if m != n // 2 + 1:
        raise ValueError(f"real_field_weights: a half spectrum of an n = {n} grid has {n // 2 + 1} columns, got {m}")
    c = torch.full((m,), 2.0, dtype=dtype, device=device)
    c[0] = 1.0
    if n % 2 == 0:
        c[-1] = 1.0
    return c / float(n * n)


def orthonormalize_tangents(dW_hat: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """QR of a bundle of tangents in the REAL-FIELD inner product <a, b> = sum_x a(x) b(x): the re-orthonormalisation of
    Benettin's method (Lyapunov spectra), of subspace and block-Krylov iterations.

    ``dW_hat``: ``(K, n, m)`` or ``(K, B, n, m)`` half spectra (``rfft2``) of real fields on an ``n x n`` grid -- the bundle
    ``tangent_bundle_step`` carries.  Returns ``(Q_hat, R)``: ``Q_hat`` of ``dW_hat``'s shape with
    ``sum_x q_j(x) q_k(x) = delta_jk`` for ``q = irfft2(Q_hat)``, and ``R`` of shape ``(K, K)`` / ``(B, K, K)``, upper triangular
    with a positive diagonal, ``dW_hat[k] = sum_j Q_hat[j] R[j, k]`` per sample.  The sum of ``log R[k, k]`` over the
    re-orthonormalisations, divided by the time, is the k-th Lyapunov exponent.

    On the half spectrum the inner product is NOT the plain complex dot product: interior columns count twice, the ky = 0
    column and (even n) the Nyquist column once, and only the real part enters (``real_field_weights``).  In those two columns
    a half spectrum also has entries no real field produces -- the part that is not Hermitian in kx, which ``irfft2`` and the
    solver's transforms drop.  The solver's own states carry one: the 2/3-rule mask keeps kx = -n/3 without its mirror image
    (n = 64: 2.5e-3 of a tangent after five steps).  That part is invisible in physical space, so it stays out of the inner
    product (it rides along through R, so that Q R is still the input).  The factorisation is a Householder QR
    (``torch.linalg.qr``) of the real, weighted ``(2 n m, K)`` matrices, so nearly parallel tangents -- the normal case, every
    tangent leans towards the leading vector -- lose no orthogonality.  Plain tensor arithmetic, run once per some tens of
    steps; not a kernel of the library."""
    if not torch.is_tensor(dW_hat) or not dW_hat.is_complex() or dW_hat.dim() not in (3, 4):
        raise ValueError("orthonormalize_tangents: expected complex half spectra of shape (K, n, m) or (K, B, n, m), got "
                         f"{tuple(getattr(dW_hat, 'shape', ()))} {getattr(dW_hat, 'dtype', None)}")
    single = dW_hat.dim() == 3
    A = dW_hat.unsqueeze(1) if single else dW_hat
    K, B, nn, m = A.shape
    if nn != n or m != n // 2 + 1:
        raise ValueError(f"orthonormalize_tangents: half spectra of an n = {n} grid are ({n}, {n // 2 + 1}), got ({nn}, {m})")
    if K > 2 * nn * m:
        raise ValueError(f"orthonormalize_tangents: {K} tangents in a space of {2 * nn * m} dimensions")
    real = dW_hat.real.dtype
    s = real_field_weights(n, m, real, dW_hat.device).sqrt()                                  # (m,)
    # the visible part: columns ky = 0 and Nyquist made Hermitian in kx, (a[i] + conj(a[-i])) / 2 -- what irfft2 sees of them
    own = [0] + ([m - 1] if n % 2 == 0 else [])
    cols = A[..., own]                                                                        # (K, B, n, 1 or 2)
    herm = 0.5 * (cols + torch.roll(cols.flip(-2), 1, -2).conj())
    V = A.clone()
    V[..., own] = herm
    M = torch.view_as_real(V * s).permute(1, 2, 3, 4, 0).reshape(B, 2 * nn * m, K)            # rows: (i, j, re / im)
    Q, R = torch.linalg.qr(M, mode="reduced")
    sign = torch.where(torch.diagonal(R, dim1=-2, dim2=-1) < 0, -1.0, 1.0).to(real)           # (B, K): positive diagonal
    Q = Q * sign.unsqueeze(-2)
    R = R * sign.unsqueeze(-1)
    Qc = torch.view_as_complex(Q.reshape(B, nn, m, 2, K).permute(4, 0, 1, 2, 3).contiguous()) / s
    # the invisible rest of the two columns, carried by the same R:  rest = (rest of Q) R
    rest = (cols - herm).permute(1, 2, 3, 0).reshape(B, nn * len(own), K)
    rest = torch.linalg.solve_triangular(R.to(dW_hat.dtype), rest, upper=True, left=False)
    Qc[..., own] += rest.reshape(B, nn, len(own), K).permute(3, 0, 1, 2)
    return (Qc[:, 0], R[0]) if single else (Qc, R)
