"""Finite-volume Navier-Stokes solver on the staggered (MAC) grid: explicit Runge-Kutta stages, each followed by a pressure
projection (torch_cfd/fvm.py ``RKStepper`` :196 and ``NavierStokes2DFVMProjection`` :334, pressure.py
``PressureProjection`` :68 / ``Pseudoinverse`` :153).

The velocity is a pair ``(ux, uy)`` of ``(n, n)`` or ``(B, n, n)`` tensors: ``ux`` at the x-faces (offset ``(1, 1/2)``),
``uy`` at the y-faces (``(1/2, 1)``), the form ``initial_conditions.filtered_velocity_field`` returns; objects with a
``.data`` tensor (the reference's ``GridVariableVector``) are accepted too.  Periodic square grids only -- all the
reference implements (its ``advect_general`` raises otherwise).

Every stage runs on the HIP kernels of ``csrc/tcfd_fvm.hip`` (C ABI ``tcfd_fvm_*``); the pressure solve uses the
project's own rfft2 / irfft2 kernels.  Gradients with respect to the velocity flow through ``forward`` / ``advance`` (any
``steps``), ``RKStepper.forward``, ``explicit_terms``, ``pressure_projection``, ``PressureProjection`` and
``get_trajectory_fvm`` when grad mode is on and ``ux`` or ``uy`` requires grad: ``fvm_autograd.py`` runs the HIP adjoint
kernels.  A stepping call under grad keeps the input of each of its K steps, ``K * 2 * B * n^2 * w`` bytes (``w`` = 8 for
fp64, 4 for fp32), until its backward has run.  A tableau whose parameters require grad raises while grad mode is on.

The advection scheme is the equation's ``convect`` argument: ``convect`` (van Leer, the default) or
``advection(interpolation.upwind | linear | lax_wendroff)``, the counterparts of the reference's ``convect`` and of an
``advect_general`` with that ``c_interpolation_fn``.  Each is one instantiation of the stage kernel and of its adjoint.

Forward mode: ``explicit_terms_jvp(u, du, dt)`` and ``tangent_step(u, du, dt, steps)`` carry a perturbation ``du`` of the
state through the tangent instantiation of the stage kernel (``k_fvm_stage_jvp``), on a tangent plan
(``tcfd_fvm_plan_set_tangent``) that steps the stacked pair ``[u; du]`` in one library call.  A dual number of
``torch.autograd.forward_ad`` given to ``forward`` / ``advance``, ``RKStepper.forward``, ``explicit_terms``, ``convect``,
``pressure_projection`` / ``PressureProjection.forward`` or ``get_trajectory_fvm`` runs the same calls; a component without a
tangent counts as a zero tangent.  Forward over reverse is not provided.

Tangent bundles: ``explicit_terms_jvp_bundle(u, dV, dt)`` and ``tangent_bundle_step(u, dV, dt, steps)`` carry K perturbations
``dV[k]`` of ONE state through the bundle instantiation of the stage kernel (``k_fvm_stage_jvp_bundle``) on a bundle plan
(``tcfd_fvm_plan_set_tangent_bundle``) that steps the stack ``[u; dV[0]; ..; dV[K-1]]`` in one library call: the state's loads,
explicit terms, flux intermediates and projections are done once, not K times, and member k has the bits of
``tangent_step(u, dV[k])``.  ``orthonormalize_velocity_tangents`` is the QR step between such calls.

Ensembles: ``viscosity`` / ``drag`` / ``forcing_scale`` given per sample (a length-B sequence or a ``(B, 1, 1)`` tensor) make the
equation an ENSEMBLE of B members.  Component ``b`` of a ``(B, n, n)`` state then runs with member ``b``'s values in every call
above that evaluates the explicit terms -- stepping, ``explicit_terms``, the tangent-linear calls and dual numbers, and reverse
mode with respect to the velocity -- on the per-sample instantiations of the same three stage kernels
(``tcfd_fvm_plan_set_ensemble``): one plan and one launch per stage for the whole sweep.  The parameters are data: one that
requires grad raises ``NotImplementedError``.  ``convect`` and the projection read no physics and are as they were.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.autograd.forward_ad as fwAD
import torch.nn as nn

from . import _lib
from . import fvm_autograd as _ad
from . import interpolation
from .equations import _ensemble_members
from .grids import Grid

_FP = {torch.float64: _lib.TCFD_C128, torch.float32: _lib.TCFD_C64}


def _tensor_of(x) -> torch.Tensor:
    return x if isinstance(x, torch.Tensor) else x.data


def _as_pair(u) -> Tuple[torch.Tensor, torch.Tensor]:
    if len(u) != 2:
        raise ValueError(f"expected a velocity pair (ux, uy), got {len(u)} components")
    ux, uy = (_tensor_of(c) for c in u)
    if ux.shape != uy.shape or ux.dtype != uy.dtype or ux.device != uy.device:
        raise ValueError(f"velocity components differ: {tuple(ux.shape)} {ux.dtype} {ux.device} vs "
                         f"{tuple(uy.shape)} {uy.dtype} {uy.device}")
    return ux, uy


def _unpack_duals(ux: torch.Tensor, uy: torch.Tensor):
    """``None`` for plain tensors; for forward-mode dual numbers ``((ux, uy), (dux, duy))``, the primals and the tangents, a
    component without a tangent counting as a zero tangent."""
    (px, tx), (py, ty) = fwAD.unpack_dual(ux), fwAD.unpack_dual(uy)
    if tx is None and ty is None:
        return None
    tx = torch.zeros_like(px) if tx is None else tx
    ty = torch.zeros_like(py) if ty is None else ty
    return (px, py), (tx, ty)


def _make_duals(out, dout):
    return tuple(fwAD.make_dual(o, d) for o, d in zip(out, dout))


def _jvp_pairs(u, du, n: int, what: str):
    """The checks the tangent-linear entry points share, before any device call: shapes and dtypes (ValueError), then
    gradients (forward over reverse is not implemented).  Returns ``((ux, uy), (dux, duy))``."""
    ux, uy = _as_pair(u)
    dux, duy = _as_pair(du)
    if dux.shape != ux.shape or dux.dtype != ux.dtype or dux.device != ux.device:
        raise ValueError(f"{what}: the tangent must have the shape and dtype of the state, got {tuple(dux.shape)} {dux.dtype} "
                         f"{dux.device} for {tuple(ux.shape)} {ux.dtype} {ux.device}")
    if ux.ndim not in (2, 3) or tuple(ux.shape[-2:]) != (n, n) or ux.dtype not in _FP:
        raise ValueError(f"{what}: expected float64 or float32 (n, n) or (B, n, n) velocity components with n = {n}, got "
                         f"{tuple(ux.shape)} {ux.dtype}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (ux, uy, dux, duy)):
        raise NotImplementedError(f"{what}: forward mode over reverse mode is not implemented -- the state or its tangent "
                                  "requires grad in grad mode; detach them or differentiate with the reverse-mode path alone")
    return (ux, uy), (dux, duy)


def _bundle_pairs(u, dV, n: int, what: str):
    """The checks the tangent-bundle entry points run before any device call: a bundle ``dV = (dVx, dVy)`` has components of
    shape ``(K,) + ux.shape`` with K >= 1 (ValueError), then those of ``_jvp_pairs``.  Returns ``((ux, uy), (dVx, dVy), K)``."""
    ux, uy = _as_pair(u)
    dvx, dvy = _as_pair(dV)
    if dvx.ndim != ux.ndim + 1 or tuple(dvx.shape[1:]) != tuple(ux.shape):
        raise ValueError(f"{what}: a bundle of K tangents has components of shape (K,) + {tuple(ux.shape)}, the state's shape "
                         f"behind the member index; got {tuple(dvx.shape)}")
    K = int(dvx.shape[0])
    if not 1 <= K <= _lib.TCFD_FVM_MAX_TANGENTS:
        raise ValueError(f"{what}: a bundle of K = {K} tangents; K runs from 1 to {_lib.TCFD_FVM_MAX_TANGENTS}")
    _jvp_pairs((ux, uy), (dvx[0], dvy[0]), n, what)
    if torch.is_grad_enabled() and (dvx.requires_grad or dvy.requires_grad):
        raise NotImplementedError(f"{what}: forward mode over reverse mode is not implemented -- the bundle requires grad in "
                                  "grad mode; detach it or differentiate with the reverse-mode path alone")
    return (ux, uy), (dvx, dvy), K


def orthonormalize_velocity_tangents(dV) -> Tuple[Tuple[torch.Tensor, torch.Tensor], torch.Tensor]:
    """QR of a bundle of velocity tangents in the cell-sum inner product ``<a, b> = sum (a_x b_x + a_y b_y)``: the
    re-orthonormalisation of Benettin's method (Lyapunov spectra), of subspace and block-Krylov iterations; the finite-volume
    counterpart of ``spectral.orthonormalize_tangents``.

    ``dV = (dVx, dVy)``: components of shape ``(K, n, n)`` or ``(K, B, n, n)`` -- the bundle ``tangent_bundle_step`` carries.
    Returns ``((Qx, Qy), R)``: Q of ``dV``'s shape with ``<Q[j], Q[k]> = delta_jk`` per sample, and ``R`` of shape ``(K, K)`` /
    ``(B, K, K)``, upper triangular with a positive diagonal, ``dV[k] = sum_j Q[j] R[j, k]``.  The sum of ``log R[k, k]`` over the
    re-orthonormalisations, divided by the time, is the k-th Lyapunov exponent.  A Householder QR (``torch.linalg.qr``) of the
    ``(2 n^2, K)`` matrices, so nearly parallel tangents -- the normal case, every tangent leans towards the leading vector --
    lose no orthogonality.  Plain tensor arithmetic on the tensors' device (the CPU included), run once per some tens of steps;
    not a kernel of the library."""
    try:
        dvx, dvy = _as_pair(dV)
    except (TypeError, AttributeError) as e:
        raise ValueError(f"orthonormalize_velocity_tangents: expected a pair (dVx, dVy) of tensors: {e}") from None
    if dvx.dim() not in (3, 4) or not dvx.is_floating_point() or dvx.shape[-1] != dvx.shape[-2]:
        raise ValueError("orthonormalize_velocity_tangents: expected real components of shape (K, n, n) or (K, B, n, n), got "
                         f"{tuple(dvx.shape)} {dvx.dtype}")
    single = dvx.dim() == 3
    ax, ay = (c.unsqueeze(1) if single else c for c in (dvx, dvy))
    K, B, n, _ = ax.shape
    if not 1 <= K <= 2 * n * n:
        raise ValueError(f"orthonormalize_velocity_tangents: {K} tangents in a space of {2 * n * n} dimensions")
    M = torch.stack([ax, ay], dim=2).reshape(K, B, 2 * n * n).permute(1, 2, 0)                # (B, 2 n^2, K); rows: (x / y, i, j)
    Q, R = torch.linalg.qr(M, mode="reduced")
    sign = torch.where(torch.diagonal(R, dim1=-2, dim2=-1) < 0, -1.0, 1.0).to(dvx.dtype)      # (B, K): positive diagonal
    Q = Q * sign.unsqueeze(-2)
    R = R * sign.unsqueeze(-1)
    Q = Q.permute(2, 0, 1).reshape(K, B, 2, n, n)
    qx, qy = Q[:, :, 0].contiguous(), Q[:, :, 1].contiguous()
    if single:
        return (qx[:, 0], qy[:, 0]), R[0]
    return (qx, qy), R


def _check_periodic(bcs) -> None:
    """``bcs``: None (periodic) or per-component boundary conditions with ``.types`` (the reference's classes)."""
    if bcs is None:
        return
    for bc in (bcs if isinstance(bcs, (list, tuple)) else [bcs]):
        types = getattr(bc, "types", None)
        if types is None:
            raise NotImplementedError(f"boundary condition {bc!r}: only periodic boundaries are implemented")
        for pair in types:
            for t in pair:
                if str(t).lower() != "periodic":
                    raise NotImplementedError(f"boundary type {t!r}: the finite-volume solver implements periodic "
                                              "boundaries only (as the reference's advect_general)")


def _square_step(grid: Grid) -> float:
    if grid.ndim != 2 or grid.shape[0] != grid.shape[1] or not math.isclose(grid.step[0], grid.step[1], rel_tol=0, abs_tol=0):
        raise NotImplementedError(f"{grid}: the finite-volume solver runs on square n x n grids with equal cell sizes")
    return grid.step[0]


# ----------------------------------------------------------------------------- advection scheme
@dataclass(frozen=True)
class Convect:
    """The advection term of the equation as a descriptor (compares and hashes by value): how the transported component
    (``c_interpolation_fn``) and the velocity (``u_interpolation_fn``) reach the faces of the control volume.  The counterpart
    of a ``convect`` function built from the reference's ``advect_general``; build one with ``advection``."""

    c_interpolation_fn: interpolation.Interpolation
    u_interpolation_fn: interpolation.Interpolation = interpolation.linear

    @property
    def scheme(self) -> int:
        """The ``TCFD_FVM_*`` value of the kernel instantiation."""
        return self.c_interpolation_fn.scheme

    def __repr__(self) -> str:
        return f"fvm.advection({self.c_interpolation_fn!r})"


def advection(c_interpolation_fn, u_interpolation_fn=interpolation.linear) -> Convect:
    """``convect`` argument of ``NavierStokes2DFVMProjection`` for advection by
    ``advect_general(c, v, u_interpolation_fn, c_interpolation_fn, dt)`` of every velocity component (torch_cfd/fvm.py:89).
    ``c_interpolation_fn``: ``interpolation.upwind``, ``linear``, ``lax_wendroff`` or
    ``apply_tvd_limiter(lax_wendroff, van_leer_limiter)``; the face velocity is interpolated linearly, as everywhere in the
    reference."""
    if not isinstance(c_interpolation_fn, interpolation.Interpolation):
        raise TypeError(f"advection: c_interpolation_fn = {c_interpolation_fn!r} is not a scheme of torch_cfd_amd.interpolation "
                        f"({_SCHEMES_TEXT}); arbitrary Python interpolation cannot run in the HIP kernels")
    if u_interpolation_fn != interpolation.linear:
        raise NotImplementedError(f"advection: u_interpolation_fn = {u_interpolation_fn!r}: the kernels interpolate the face "
                                  "velocity with interpolation.linear only")
    return Convect(c_interpolation_fn, interpolation.linear)


_SCHEMES_TEXT = ("interpolation.upwind, interpolation.linear, interpolation.lax_wendroff, "
                 "interpolation.apply_tvd_limiter(interpolation.lax_wendroff, interpolation.van_leer_limiter)")

# van Leer: the counterpart of the reference's module-level ``convect`` (advect_van_leer_using_limiters of every component)
convect = _VAN_LEER_CONVECT = advection(interpolation.apply_tvd_limiter(interpolation.lax_wendroff, interpolation.van_leer_limiter))


def _as_convect(c) -> Convect:
    if c is None:
        return _VAN_LEER_CONVECT
    if isinstance(c, Convect):
        return c
    raise TypeError(f"convect = {c!r}: arbitrary Python advection cannot run in the HIP kernels of the finite-volume solver. "
                    f"Pass fvm.convect (van Leer, the default) or fvm.advection(c) with c one of {_SCHEMES_TEXT}.")


# ----------------------------------------------------------------------------- tableau
class RKStepper(nn.Module):
    """Explicit Runge-Kutta tableau ``{"a": rows, "b": weights}`` (torch_cfd/fvm.py:196).

    The parameters are stored as the reference stores them -- ``params.a.{i}`` (row i = stage i + 1), ``params.b`` --
    in ``dtype``, float32 by default.  The stage weights are formed as the reference forms them, ``dt * a_ij`` in the
    parameters' precision: an fp64 run of classic RK4 steps with ``b = float32(1/6)``, as there.  Zero entries are
    skipped.  The parameters require grad only with ``requires_grad=True``; gradients with respect to them are not
    implemented (the step raises in grad mode), those with respect to the velocity are."""

    _METHOD_MAP = {
        "forward_euler": {"a": [], "b": [1.0]},
        "midpoint": {"a": [[1 / 2]], "b": [0, 1.0]},
        "heun_rk2": {"a": [[1.0]], "b": [1 / 2, 1 / 2]},
        "classic_rk4": {
            "a": [[1 / 2], [0.0, 1 / 2], [0.0, 0.0, 1.0]],
            "b": [1 / 6, 1 / 3, 1 / 3, 1 / 6],
        },
    }
    MAX_STAGES = 4

    def __init__(self, tableau: Optional[Dict[str, List]] = None, method: Optional[str] = None,
                 dtype: Optional[torch.dtype] = torch.float32, requires_grad: bool = False, **kwargs):
        super().__init__()
        self.dtype = dtype
        self.requires_grad = requires_grad
        if tableau is not None:
            self._tableau, self._method = tableau, None
        else:
            if method not in self._METHOD_MAP:
                raise ValueError(f"Unknown RK method: {method}")
            self._tableau, self._method = self._METHOD_MAP[method], method
        self._set_params(self._tableau)

    @property
    def method(self):
        return self._method

    @property
    def tableau(self):
        return self._tableau

    @property
    def num_stages(self) -> int:
        return len(self.params["b"])

    def _set_params(self, tableau: Dict[str, List]) -> None:
        a, b = tableau["a"], tableau["b"]
        if len(a) + 1 != len(b):
            raise ValueError("Inconsistent Butcher tableau: len(a) + 1 != len(b)")
        for i, row in enumerate(a):
            if len(row) != i + 1:
                raise ValueError(f"Inconsistent Butcher tableau: row {i} of a has {len(row)} entries, an explicit "
                                 f"tableau has {i + 1} there")
        if len(b) > self.MAX_STAGES:
            raise ValueError(f"{len(b)} stages: the finite-volume kernels take explicit tableaux of up to "
                             f"{self.MAX_STAGES} stages")
        self.params = nn.ParameterDict()
        self.params["a"] = nn.ParameterList()
        for row in a:
            self.params["a"].append(nn.Parameter(torch.tensor(row, dtype=self.dtype), requires_grad=self.requires_grad))
        self.params["b"] = nn.Parameter(torch.tensor(b, dtype=self.dtype), requires_grad=self.requires_grad)

    @classmethod
    def from_method(cls, method: str = "forward_euler", requires_grad: bool = False, **kwargs):
        return cls(method=method, requires_grad=requires_grad, **kwargs)

    def _check_no_grad(self) -> None:
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("RKStepper: the finite-volume step has no gradients with respect to its tableau, whose "
                                      "parameters require grad. Run under torch.no_grad() or build the stepper with "
                                      "requires_grad=False (gradients with respect to the velocity are supported).")

    def weights(self, dt: float) -> Tuple[List[float], List[float]]:
        """(a, b) as the kernels take them: ``a`` row-major (stages x stages, row i = stage i) and ``b``, each entry
        ``dt * coefficient`` evaluated as the reference does (in the parameters' dtype), 0 for a skipped term."""
        s = self.num_stages
        a = [0.0] * (s * s)
        with torch.no_grad():
            alpha, beta = self.params["a"], self.params["b"]
            for i in range(1, s):
                for j in range(i):
                    if alpha[i - 1][j] != 0:
                        a[i * s + j] = float(dt * alpha[i - 1][j])
            b = [float(dt * beta[j]) if beta[j] != 0 else 0.0 for j in range(s)]
        return a, b

    def forward(self, u0, dt: float, equation: "NavierStokes2DFVMProjection"):
        """One step of ``equation`` (the reference's calling convention ``step_fn.forward(v, dt, equation=ns2d)``)."""
        return equation.advance(u0, dt, steps=1, solver=self)


# ----------------------------------------------------------------------------- device plan
def _require_entry(lib, name: str, what: str) -> None:
    """An entry point added without a new ABI number: a library built before it loads, but lacks it."""
    if not hasattr(lib, name):
        raise _lib.TcfdError(f"{_lib.LIB_PATH} was built before {what} ({name}) were added: rebuild it with "
                             "torch_cfd_amd._lib.build_library(force=True)")


class _FvmPlan:
    """Owns one ``tcfd_fvm_plan`` (inverse-eigenvalue and forcing tables) + a workspace."""

    def __init__(self, n: int, dtype: torch.dtype, device: torch.device, h: float, nu: float, drag: float,
                 inverse: torch.Tensor, force: Optional[Tuple[torch.Tensor, torch.Tensor]],
                 scheme: int = _lib.TCFD_FVM_VAN_LEER, tangent: bool = False, members=None, bundle: int = 0):
        self.lib = _lib.load()
        self.n, self.dtype, self.device = n, dtype, torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TcfdError("torch-cfd_amd runs on HIP devices only (no CPU fallback); got " + str(device))
        inv = torch.view_as_real(inverse.detach().to("cpu", torch.complex128).contiguous()).contiguous()
        assert inv.shape == (n, n // 2 + 1, 2)
        keep = [inv]
        fx = fy = None
        if force is not None:
            fx_t, fy_t = (f.detach().to("cpu", torch.float64).expand(n, n).contiguous() for f in force)
            keep += [fx_t, fy_t]
            fx, fy = _lib.dptr_of_tensor(fx_t), _lib.dptr_of_tensor(fy_t)
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_plan_create(ctypes.byref(handle), n, _FP[dtype], float(h), float(nu), float(drag),
                                               _lib.dptr_of_tensor(inv), fx, fy)
        _lib.check(rc, "tcfd_fvm_plan_create")
        self.handle = handle
        self._ws: Optional[torch.Tensor] = None
        self._finalizer = weakref.finalize(self, self.lib.tcfd_fvm_plan_destroy, handle)
        self.scheme = int(scheme)   # fixed for the plan's life: a pending backward holds the plan and so its scheme
        _lib.check(self.lib.tcfd_fvm_plan_set_advection(handle, self.scheme), "tcfd_fvm_plan_set_advection")
        self.tangent = bool(tangent)   # a tangent plan steps pairs [u; du]: its calls go through the *_pair methods below
        if self.tangent:
            _lib.check(self.lib.tcfd_fvm_plan_set_tangent(handle, 1), "tcfd_fvm_plan_set_tangent")
        self.bundle = int(bundle)   # K > 0: a bundle plan steps [u; du_0 .. du_{K-1}]: its calls go through the *_bundle methods
        if self.bundle:
            _require_entry(self.lib, "tcfd_fvm_plan_set_tangent_bundle", "tangent bundles")
            _lib.check(self.lib.tcfd_fvm_plan_set_tangent_bundle(handle, self.bundle), "tcfd_fvm_plan_set_tangent_bundle")
        self.members = 0   # B of an ensemble plan: every call but project then takes B fields (a tangent plan: 2 B; a bundle: (1 + K) B)
        if members is not None:
            self.set_ensemble(*members)

    def set_ensemble(self, nu_over_density=None, drag=None, forcing_scale=None) -> None:
        """Per-sample physics (``tcfd_fvm_plan_set_ensemble``): field b of every later call runs with ``nu_over_density[b]``,
        ``drag[b]`` (None: the plan's scalar drag) and ``forcing_scale[b]`` times the plan's forcing (None: 1).  Sequences of one
        length B; no ``nu_over_density`` clears the table and the plan is scalar again."""
        if not hasattr(self.lib, "tcfd_fvm_plan_set_ensemble"):   # added without a new ABI number: a stale library loads, but lacks it
            raise _lib.TcfdError(f"{_lib.LIB_PATH} was built before per-sample parameters (tcfd_fvm_plan_set_ensemble) were "
                                 "added: rebuild it with torch_cfd_amd._lib.build_library(force=True)")
        count = 0 if nu_over_density is None else len(nu_over_density)
        for name, v in (("drag", drag), ("forcing_scale", forcing_scale)):
            if count and v is not None and len(v) != count:
                raise ValueError(f"set_ensemble: {count} viscosities, {len(v)} values of {name}")
        arr = lambda v: _lib.darray(v) if count and v is not None else None
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_plan_set_ensemble(self.handle, count, arr(nu_over_density), arr(drag), arr(forcing_scale))
        _lib.check(rc, "tcfd_fvm_plan_set_ensemble")
        self.members = count

    def workspace(self, batch: int, need: Optional[int] = None) -> torch.Tensor:
        """At least ``need`` bytes (default: what ``tcfd_fvm_step`` needs for ``batch``)."""
        if need is None:
            need = self.lib.tcfd_fvm_workspace_bytes(self.handle, batch)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _prep(self, ux, uy):
        if not ux.is_cuda or ux.device != self.device:
            raise _lib.TcfdError(f"expected tensors on {self.device} (torch-cfd_amd has no CPU fallback), got {ux.device}")
        if ux.shape[-2:] != (self.n, self.n) or ux.ndim not in (2, 3):
            raise ValueError(f"expected (n, n) or (B, n, n) velocity components with n = {self.n}, got {tuple(ux.shape)}")
        ux = ux.detach().to(self.dtype).contiguous()
        uy = uy.detach().to(self.dtype).contiguous()
        return ux, uy, ux.numel() // (self.n * self.n)

    def explicit_terms(self, ux, uy, dt: float):
        ux, uy, batch = self._prep(ux, uy)
        kx, ky = torch.empty_like(ux), torch.empty_like(uy)
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_explicit_terms(self.handle, ux.data_ptr(), uy.data_ptr(), kx.data_ptr(), ky.data_ptr(),
                                                  batch, float(dt), self._stream())
        _lib.check(rc, "tcfd_fvm_explicit_terms")
        return kx, ky

    def project(self, ux, uy):
        ux, uy, batch = self._prep(ux, uy)
        ox, oy = torch.empty_like(ux), torch.empty_like(uy)
        ws = self.workspace(batch)
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_project(self.handle, ux.data_ptr(), uy.data_ptr(), ox.data_ptr(), oy.data_ptr(), batch,
                                           ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(rc, "tcfd_fvm_project")
        return ox, oy

    def step(self, ux, uy, dt: float, a: Sequence[float], b: Sequence[float], steps: int):
        ux, uy, batch = self._prep(ux, uy)
        ox, oy = torch.empty_like(ux), torch.empty_like(uy)
        ws = self.workspace(batch)
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_step(self.handle, ux.data_ptr(), uy.data_ptr(), ox.data_ptr(), oy.data_ptr(), batch,
                                        int(steps), len(b), _lib.darray(a) if len(a) else None, _lib.darray(b), float(dt),
                                        ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(rc, "tcfd_fvm_step")
        return ox, oy

    # ---- forward mode: the stacked pair [u; du] of a tangent plan (project: of any plan, the projection being linear)
    @staticmethod
    def _stack(u, du):
        return torch.cat([u.reshape((-1,) + u.shape[-2:]), du.reshape((-1,) + du.shape[-2:])])

    @staticmethod
    def _split(ox, oy, shape):
        b = ox.shape[0] // 2
        return (ox[:b].reshape(shape), oy[:b].reshape(shape)), (ox[b:].reshape(shape), oy[b:].reshape(shape))

    def explicit_terms_pair(self, ux, uy, dux, duy, dt: float):
        """``((kx, ky), (dkx, dky))`` = ``(F(u), J_F(u) du)``, one launch of the tangent stage kernel."""
        assert self.tangent
        return self._split(*self.explicit_terms(self._stack(ux, dux), self._stack(uy, duy), dt), ux.shape)

    def step_pair(self, ux, uy, dux, duy, dt: float, a: Sequence[float], b: Sequence[float], steps: int):
        """``steps`` RK steps of the state and of its tangent in one library call."""
        assert self.tangent
        return self._split(*self.step(self._stack(ux, dux), self._stack(uy, duy), dt, a, b, steps), ux.shape)

    def project_pair(self, ux, uy, dux, duy):
        return self._split(*self.project(self._stack(ux, dux), self._stack(uy, duy)), ux.shape)

    # ---- a bundle plan: the state and its K tangents stacked, [u; du_0; ..; du_{K-1}], tangent k (1 + k) B fields in
    def _stack_bundle(self, u, dv):
        return torch.cat([u.reshape((-1,) + u.shape[-2:]), dv.reshape((-1,) + dv.shape[-2:])])

    def _split_bundle(self, ox, oy, shape):
        b = ox.shape[0] // (1 + self.bundle)
        tshape = (self.bundle,) + tuple(shape)
        return (ox[:b].reshape(shape), oy[:b].reshape(shape)), (ox[b:].reshape(tshape), oy[b:].reshape(tshape))

    def explicit_terms_bundle(self, ux, uy, dvx, dvy, dt: float):
        """``((kx, ky), (dKx, dKy))`` = ``(F(u), [J_F(u) dV[k]])``, one launch of the bundle stage kernel."""
        assert self.bundle and dvx.shape[0] == self.bundle
        return self._split_bundle(*self.explicit_terms(self._stack_bundle(ux, dvx), self._stack_bundle(uy, dvy), dt), ux.shape)

    def step_bundle(self, ux, uy, dvx, dvy, dt: float, a: Sequence[float], b: Sequence[float], steps: int):
        """``steps`` RK steps of the state and of its K tangents in one library call."""
        assert self.bundle and dvx.shape[0] == self.bundle
        return self._split_bundle(*self.step(self._stack_bundle(ux, dvx), self._stack_bundle(uy, dvy), dt, a, b, steps), ux.shape)

    # ---- reverse mode (fvm_autograd.py)
    def explicit_terms_vjp(self, ux, uy, gx, gy, dt: float):
        ux, uy, batch = self._prep(ux, uy)
        gx, gy, _ = self._prep(gx, gy)
        ox, oy = torch.empty_like(ux), torch.empty_like(uy)
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_explicit_terms_vjp(self.handle, ux.data_ptr(), uy.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                                                      ox.data_ptr(), oy.data_ptr(), batch, float(dt), self._stream())
        _lib.check(rc, "tcfd_fvm_explicit_terms_vjp")
        return ox, oy

    def step_saving(self, ux, uy, dt: float, a: Sequence[float], b: Sequence[float], steps: int):
        """``step`` as ``steps`` one-step calls (bit-equal to one call of ``steps``), keeping the input of each:
        returns ``(saved, ux_out, uy_out)`` with ``saved`` of shape ``(steps, 2, *ux.shape)``."""
        ux, uy, batch = self._prep(ux, uy)
        saved = torch.empty((steps, 2) + tuple(ux.shape), dtype=ux.dtype, device=ux.device)
        ox, oy = torch.empty_like(ux), torch.empty_like(uy)
        if steps == 0:
            ox.copy_(ux)
            oy.copy_(uy)
            return saved, ox, oy
        saved[0, 0].copy_(ux)
        saved[0, 1].copy_(uy)
        ws = self.workspace(batch)
        ca, cb = (_lib.darray(a) if len(a) else None), _lib.darray(b)
        with torch.cuda.device(self.device):
            for s in range(steps):
                tx, ty = (saved[s + 1, 0], saved[s + 1, 1]) if s + 1 < steps else (ox, oy)
                rc = self.lib.tcfd_fvm_step(self.handle, saved[s, 0].data_ptr(), saved[s, 1].data_ptr(), tx.data_ptr(),
                                            ty.data_ptr(), batch, 1, len(b), ca, cb, float(dt), ws.data_ptr(), ws.numel(),
                                            self._stream())
                _lib.check(rc, "tcfd_fvm_step")
        return saved, ox, oy

    def step_vjp(self, saved, gx, gy, dt: float, a: Sequence[float], b: Sequence[float]):
        """Cotangent of the input of ``step_saving``'s steps from that of their result (``saved``: its record)."""
        gx, gy, batch = self._prep(gx, gy)
        ox, oy = torch.empty_like(gx), torch.empty_like(gy)
        steps = saved.shape[0]
        ws = self.workspace(batch, self.lib.tcfd_fvm_step_vjp_workspace_bytes(self.handle, batch))
        with torch.cuda.device(self.device):
            rc = self.lib.tcfd_fvm_step_vjp(self.handle, saved.data_ptr() if steps else None, gx.data_ptr(), gy.data_ptr(),
                                            ox.data_ptr(), oy.data_ptr(), batch, int(steps), len(b),
                                            _lib.darray(a) if len(a) else None, _lib.darray(b), float(dt), ws.data_ptr(),
                                            ws.numel(), self._stream())
        _lib.check(rc, "tcfd_fvm_step_vjp")
        return ox, oy


# ----------------------------------------------------------------------------- pressure projection
def laplacian_matrix(n: int, step: float, dtype=None) -> torch.Tensor:
    """Dense periodic 1-D finite-difference Laplacian (torch_cfd/finite_differences.py:167-193)."""
    column = torch.zeros(n, dtype=dtype)
    column[0] = -2 / step**2
    column[1] = column[-1] = 1 / step**2
    idx = (n - torch.arange(n)[None].T + torch.arange(n)[None]) % n
    return torch.gather(column[None, ...].expand(n, -1), 1, idx)


def _circulant_eigenvalues(n: int, step: float, half: bool, dtype) -> torch.Tensor:
    """Eigenvalues of the periodic FD Laplacian = the DFT of its first column, in closed form:
    ``-2 / h^2 + 2 cos(2 pi k / n) / h^2`` (k < n, or k <= n / 2 for the half spectrum)."""
    k = torch.arange(n // 2 + 1 if half else n, dtype=torch.float64)
    lam = (-2 / step**2) + (2 / step**2) * torch.cos(2 * math.pi * k / n)
    lam[0] = 0.0   # the column sums to zero exactly: -2/h^2 + 1/h^2 + 1/h^2
    return lam.to(dtype)


class Pseudoinverse(nn.Module):
    """Pseudo-inverse of the periodic FD Laplacian by rfft2 diagonalisation (pressure.py:153, implementation "rfft").
    Buffers as the reference's: ``laplacians`` (2, n, n), ``inverse`` (n, n/2 + 1) complex, ``eigenvectors``.
    The eigenvalue cut-off is ``10 eps(dtype)`` -- float32 by default whatever the field precision, as there."""

    def __init__(self, grid: Grid, bc=None, dtype: torch.dtype = torch.float32, laplacians: Optional[torch.Tensor] = None,
                 cutoff: Optional[float] = None, **unused):
        super().__init__()
        _check_periodic(bc)
        self.grid = grid
        self.cutoff = cutoff or 10 * torch.finfo(dtype).eps
        n, h = grid.shape[0], _square_step(grid)
        if n % 2:
            raise NotImplementedError(f"n = {n}: the rfft pseudo-inverse needs an even grid")
        if laplacians is None:
            laplacians = torch.stack([laplacian_matrix(m, s) for m, s in zip(grid.shape, grid.step)])
        self.register_buffer("laplacians", laplacians, persistent=True)
        real = laplacians.dtype
        cplx = torch.complex128 if real == torch.float64 else torch.complex64
        summed = _circulant_eigenvalues(n, h, False, real)[:, None] + _circulant_eigenvalues(n, h, True, real)[None, :]
        summed = summed.to(cplx)
        inverse = torch.where(torch.abs(summed) > self.cutoff, 1 / summed, 0)
        self.register_buffer("inverse", inverse, persistent=True)
        self.register_buffer("eigenvectors", torch.tensor([1.0] * grid.ndim), persistent=True)


class PressureProjection(nn.Module):
    """``u - grad q`` with ``q = pinv(L) div u``: backward-difference divergence, pseudo-inverse by the HIP rfft2 /
    irfft2 kernels, forward-difference gradient (pressure.py:68-106).  Periodic boundaries only."""

    def __init__(self, grid: Grid, bc=None, dtype: torch.dtype = torch.float32, laplacians: Optional[torch.Tensor] = None,
                 **unused):
        super().__init__()
        _check_periodic(bc)
        self.grid = grid
        self.dtype = dtype
        if laplacians is None:
            laplacians = torch.stack([laplacian_matrix(m, s) for m, s in zip(grid.shape, grid.step)])
        self.register_buffer("laplacians", laplacians, persistent=True)
        self.solver = Pseudoinverse(grid, bc, dtype=dtype, laplacians=self.laplacians)
        self._plans: Dict[tuple, _FvmPlan] = {}

    def _plan(self, dtype, device) -> _FvmPlan:
        inv = self.solver.inverse
        key = (torch.device(device), dtype, id(inv), inv._version)
        plan = self._plans.get(key)
        if plan is None:
            self._plans.clear()
            plan = _FvmPlan(self.grid.shape[0], dtype, device, _square_step(self.grid), 0.0, 0.0, inv, None)
            self._plans[key] = plan
        return plan

    def forward(self, v):
        ux, uy = _as_pair(v)
        duals = _unpack_duals(ux, uy)
        if duals is not None:   # forward mode: the projection is linear, so the stacked pair runs through it as it is
            (ux, uy), (dux, duy) = _jvp_pairs(*duals, self.grid.shape[0], "pressure_projection")
            return _make_duals(*self._plan(ux.dtype, ux.device).project_pair(ux, uy, dux, duy))
        plan = self._plan(ux.dtype, ux.device)
        if _ad.wants_grad(ux, uy):
            return _ad.ProjectFn.apply(plan, ux, uy)
        return plan.project(ux, uy)


# ----------------------------------------------------------------------------- the equation
class NavierStokes2DFVMProjection(nn.Module):
    """Incompressible Navier-Stokes on the MAC grid: explicit RK stages of
    ``du/dt = -(u . grad) u + nu / density lap u + forcing / density - drag u``, each stage state and the result
    projected onto discretely divergence-free fields (torch_cfd/fvm.py:334).  ``convect`` is the advection scheme:
    ``fvm.convect`` (van Leer; also ``None``) or ``fvm.advection(interpolation.upwind | linear | lax_wendroff)``; any other
    callable raises ``TypeError``, since Python advection cannot run in the kernels.

    ``forward(u, dt, steps=1)`` runs ``steps`` steps of ``solver`` (an ``RKStepper``) in one device call and returns the
    pair ``(ux, uy)``; ``explicit_terms(u, dt)`` and ``pressure_projection(u)`` are the two halves on their own, and
    ``convect(u, dt)`` is the advection term alone.  All four
    are differentiable with respect to ``u`` (``fvm_autograd.py``); under grad, ``forward`` runs one device call per step
    and keeps each step's input, ``steps * 2 * B * n^2 * w`` bytes, for its backward."""

    def __init__(self, viscosity, grid: Grid, bcs=None, drag=0.0, density: float = 1.0, forcing=None,
                 solver: Optional[RKStepper] = None, convect: Optional[Convect] = _VAN_LEER_CONVECT, forcing_scale=None,
                 **kwargs):
        """``viscosity`` / ``drag``: a float -- one physics for every field, as the reference -- or per-sample values: a 1-D
        sequence / tensor of length B or a ``(B, 1, 1)`` tensor.  ``forcing_scale``: a float or a length-B sequence; sample b is
        forced by ``forcing_scale[b] * forcing``.  Any per-sample argument makes the equation an ENSEMBLE of B members (single
        values are repeated): component b of a ``(B, n, n)`` state runs with member b's values.  ``density`` is one value."""
        super().__init__()
        _check_periodic(bcs)
        _square_step(grid)
        if forcing_scale is not None and forcing is None:
            raise ValueError("forcing_scale without a forcing: there is nothing to scale")
        members = _ensemble_members(viscosity, drag, forcing_scale)
        self._ens_count = 0 if members is None else int(members[0].numel())
        if members is None:   # the scalar equation: attributes and plan as they always were
            self.viscosity, self.drag, self.forcing_scale = viscosity, drag, forcing_scale
        else:                 # per-sample BUFFERS in the reference's broadcasting shape
            for name, v in zip(("viscosity", "drag", "forcing_scale"), members):
                self.register_buffer(name, v.reshape(-1, 1, 1))
        self.density = density
        self.grid = grid
        self.bcs = bcs
        self.forcing = forcing
        self.solver = solver
        self.advection = _as_convect(convect)
        self._projection = PressureProjection(grid=grid)
        self._plans: Dict[tuple, _FvmPlan] = {}
        self._convect_plans: Dict[tuple, _FvmPlan] = {}
        self._tangent_plans: Dict[tuple, _FvmPlan] = {}           # the tangent variants of the two: plain calls never see them
        self._convect_tangent_plans: Dict[tuple, _FvmPlan] = {}
        self._bundle_plans: Dict[tuple, Dict[int, _FvmPlan]] = {}  # key -> {K: the bundle plan of K tangents}

    def _force_tables(self):
        """(fx, fy) / density at the staggered offsets, sampled once per plan (the forcing is state independent)."""
        if self.forcing is None:
            return None
        f = self.forcing(self.grid, None)
        tables = tuple(_tensor_of(c).detach().to("cpu", torch.float64) / self.density for c in f)
        if not self._ens_count and self.forcing_scale is not None:   # one amplitude for every field
            tables = tuple(float(self.forcing_scale) * t for t in tables)
        return tables

    # -- per-sample parameters
    def _member_tables(self):
        return (self.viscosity, self.drag, self.forcing_scale)

    def _members(self):
        """None for the scalar equation, else ``(nu / density, drag, forcing_scale)`` of the B members as lists (no forcing
        scales without a forcing: the plan has nothing to scale)."""
        if not self._ens_count:
            return None
        nu, drag, fs = (t.detach().reshape(-1).to("cpu", torch.float64) for t in self._member_tables())
        return (nu / self.density).tolist(), drag.tolist(), (fs.tolist() if self.forcing is not None else None)

    def _check_members(self, ux: torch.Tensor, what: str) -> None:
        """An ensemble steps exactly its B members, one ``(n, n)`` field each."""
        if self._ens_count and (ux.ndim != 3 or ux.shape[0] != self._ens_count):
            raise ValueError(f"{what}: an ensemble of B = {self._ens_count} members (viscosity / drag / forcing_scale given per "
                             f"sample) takes (B, n, n) velocity components with B = {self._ens_count}, got {tuple(ux.shape)}")

    def _plan_key(self, dtype, device) -> tuple:
        inv = self._projection.solver.inverse
        fkey = None if self.forcing is None else getattr(self.forcing, "fingerprint", lambda: id(self.forcing))()
        if not self._ens_count and self.forcing_scale is not None:   # one amplitude for every field: part of the forcing table
            fkey = (fkey, float(self.forcing_scale))
        if self._ens_count:   # the member values: a changed buffer (another storage, an in-place write) builds a new plan
            for t in self._member_tables():
                if t.requires_grad:
                    raise NotImplementedError("per-sample parameters are data: a viscosity / drag / forcing_scale that requires "
                                              "grad is not implemented (gradients with respect to the parameters are out of scope)")
            return (torch.device(device), dtype, self.grid.shape[0], float(self.density), fkey, id(inv), inv._version,
                    self.advection.scheme) + tuple((t.data_ptr(), t._version) for t in self._member_tables())
        return (torch.device(device), dtype, self.grid.shape[0], float(self.viscosity), float(self.density), float(self.drag),
                fkey, id(inv), inv._version, self.advection.scheme)

    def _plan(self, dtype, device, tangent: bool = False) -> _FvmPlan:
        key = self._plan_key(dtype, device)
        plans = self._tangent_plans if tangent else self._plans
        plan = plans.get(key)
        if plan is None:
            plans.clear()
            members = self._members()
            nu, drag = (members[0][0], members[1][0]) if members else (self.viscosity / self.density, self.drag)
            plan = _FvmPlan(self.grid.shape[0], dtype, device, _square_step(self.grid), nu, drag,
                            self._projection.solver.inverse, self._force_tables(), self.advection.scheme, tangent=tangent,
                            members=members)
            plans[key] = plan
        return plan

    def _bundle_plan(self, dtype, device, K: int) -> _FvmPlan:
        """The bundle plan of K tangents per state (``tcfd_fvm_plan_set_tangent_bundle``), cached per K under the key of
        ``_plans`` / ``_tangent_plans``; a changed key drops the plans of every K."""
        key = self._plan_key(dtype, device)
        per_k = self._bundle_plans.get(key)
        if per_k is None:
            self._bundle_plans.clear()
            per_k = self._bundle_plans[key] = {}
        plan = per_k.get(K)
        if plan is None:
            members = self._members()
            nu, drag = (members[0][0], members[1][0]) if members else (self.viscosity / self.density, self.drag)
            plan = per_k[K] = _FvmPlan(self.grid.shape[0], dtype, device, _square_step(self.grid), nu, drag,
                                       self._projection.solver.inverse, self._force_tables(), self.advection.scheme,
                                       members=members, bundle=K)
        return plan

    def _convect_plan(self, dtype, device, tangent: bool = False) -> _FvmPlan:
        """The plan of the advection term alone: no viscosity, no drag, no forcing.  A second full plan, created at the first
        ``convect`` call: it uploads the inverse-eigenvalue table again and owns a transform plan it never runs, and a
        differentiable call holds it until its backward (the autograd node keeps the reference, so clearing the cache
        below is safe)."""
        inv = self._projection.solver.inverse
        key = (torch.device(device), dtype, self.grid.shape[0], id(inv), inv._version, self.advection.scheme)
        plans = self._convect_tangent_plans if tangent else self._convect_plans
        plan = plans.get(key)
        if plan is None:
            plans.clear()
            plan = _FvmPlan(self.grid.shape[0], dtype, device, _square_step(self.grid), 0.0, 0.0, inv, None,
                            self.advection.scheme, tangent=tangent)
            plans[key] = plan
        return plan

    def convect(self, u, dt: float):
        """The advection term ``-(u . grad) u`` of the equation's scheme as a pair ``(ux, uy)`` (the reference's
        ``self.convect(v, dt)``): the explicit-terms kernel on a plan without viscosity, drag and forcing."""
        ux, uy = _as_pair(u)
        duals = _unpack_duals(ux, uy)
        if duals is not None:   # forward mode: the tangent variant of the advection-only plan
            (ux, uy), (dux, duy) = _jvp_pairs(*duals, self.grid.shape[0], "convect")
            return _make_duals(*self._convect_plan(ux.dtype, ux.device, tangent=True).explicit_terms_pair(ux, uy, dux, duy, dt))
        plan = self._convect_plan(ux.dtype, ux.device)
        if _ad.wants_grad(ux, uy):
            return _ad.ExplicitTermsFn.apply(plan, dt, ux, uy)
        return plan.explicit_terms(ux, uy, dt)

    # -- forward mode: the tangent-linear model on the tangent stage kernel (a tangent plan, tcfd_fvm_plan_set_tangent)
    def explicit_terms_jvp(self, u, du, dt: float):
        """``((kx, ky), (dkx, dky))``: the explicit terms ``F(u)`` and their directional derivative ``J_F(u) du`` along the
        pair ``du`` (shapes and dtype of ``u``), one fused launch.  The tangent carries no forcing."""
        (ux, uy), (dux, duy) = _jvp_pairs(u, du, self.grid.shape[0], "explicit_terms_jvp")
        self._check_members(ux, "explicit_terms_jvp")
        return self._plan(ux.dtype, ux.device, tangent=True).explicit_terms_pair(ux, uy, dux, duy, dt)

    def _tangent_steps(self, u, du, dt: float, steps: int, solver: Optional[RKStepper]):
        if solver is None:
            raise ValueError("NavierStokes2DFVMProjection: no RKStepper (pass solver=RKStepper.from_method(...))")
        (ux, uy), (dux, duy) = _jvp_pairs(u, du, self.grid.shape[0], "tangent_step")
        self._check_members(ux, "tangent_step")
        solver._check_no_grad()
        a, b = solver.weights(dt)
        return self._plan(ux.dtype, ux.device, tangent=True).step_pair(ux, uy, dux, duy, dt, a, b, steps)

    def tangent_step(self, u, du, dt: float, steps: int = 1):
        """``steps`` steps of the equation's solver on the state AND on a perturbation of it: returns
        ``((ux, uy), (dux, duy))`` with ``du_new = d(u_new)/d(u) . du`` (the tangent-linear model), all stages and
        projections of all steps in one library call.  ``(n, n)`` or ``(B, n, n)`` components."""
        return self._tangent_steps(u, du, dt, steps, self.solver)

    # -- a bundle of K tangents per state on the bundle stage kernel (a bundle plan, tcfd_fvm_plan_set_tangent_bundle)
    def explicit_terms_jvp_bundle(self, u, dV, dt: float):
        """``((kx, ky), (dKx, dKy))``: the explicit terms ``F(u)`` and ``J_F(u) dV[k]`` for the K members of the bundle
        ``dV = (dVx, dVy)`` (components of shape ``(K,) + ux.shape``), one fused launch.  Member k has the bits of
        ``explicit_terms_jvp(u, dV[k], dt)``."""
        (ux, uy), (dvx, dvy), K = _bundle_pairs(u, dV, self.grid.shape[0], "explicit_terms_jvp_bundle")
        self._check_members(ux, "explicit_terms_jvp_bundle")
        return self._bundle_plan(ux.dtype, ux.device, K).explicit_terms_bundle(ux, uy, dvx, dvy, dt)

    def tangent_bundle_step(self, u, dV, dt: float, steps: int = 1):
        """``steps`` steps of the equation's solver on the state AND on K perturbations of it, ``dV = (dVx, dVy)`` with
        components of shape ``(K,) + ux.shape``: returns ``((ux, uy), (dUx, dUy))`` with ``dU[k] = d(u_new)/d(u) . dV[k]``, all
        stages and projections of all steps in one library call.  What K calls of ``tangent_step`` on the same state compute --
        member k has their bits -- with the state's share of every stage and its projections done once (Lyapunov spectra with
        ``orthonormalize_velocity_tangents``, block Krylov, several Gauss-Newton directions)."""
        if self.solver is None:
            raise ValueError("NavierStokes2DFVMProjection: no RKStepper (pass solver=RKStepper.from_method(...))")
        (ux, uy), (dvx, dvy), K = _bundle_pairs(u, dV, self.grid.shape[0], "tangent_bundle_step")
        self._check_members(ux, "tangent_bundle_step")
        self.solver._check_no_grad()
        a, b = self.solver.weights(dt)
        return self._bundle_plan(ux.dtype, ux.device, K).step_bundle(ux, uy, dvx, dvy, dt, a, b, steps)

    def explicit_terms(self, u, dt: float):
        ux, uy = _as_pair(u)
        duals = _unpack_duals(ux, uy)
        if duals is not None:
            return _make_duals(*self.explicit_terms_jvp(*duals, dt))
        self._check_members(ux, "explicit_terms")
        plan = self._plan(ux.dtype, ux.device)
        if _ad.wants_grad(ux, uy):
            return _ad.ExplicitTermsFn.apply(plan, dt, ux, uy)
        return plan.explicit_terms(ux, uy, dt)

    def pressure_projection(self, u):
        return self._projection(u)

    def advance(self, u, dt: float, steps: int = 1, solver: Optional[RKStepper] = None):
        solver = self.solver if solver is None else solver
        if solver is None:
            raise ValueError("NavierStokes2DFVMProjection: no RKStepper (pass solver=RKStepper.from_method(...))")
        ux, uy = _as_pair(u)
        duals = _unpack_duals(ux, uy)
        if duals is not None:   # forward-mode dual numbers: the tangent-linear step carries them
            return _make_duals(*self._tangent_steps(*duals, dt, steps, solver))
        solver._check_no_grad()
        self._check_members(ux, "advance")
        a, b = solver.weights(dt)
        plan = self._plan(ux.dtype, ux.device)
        if _ad.wants_grad(ux, uy):
            return _ad.StepFn.apply(plan, dt, a, b, steps, ux, uy)
        return plan.step(ux, uy, dt, a, b, steps)

    def forward(self, u, dt: float, steps: int = 1):
        return self.advance(u, dt, steps=steps)


def get_trajectory_fvm(equation: NavierStokes2DFVMProjection, u0, dt: float, num_steps: int, record_every_steps: int):
    """Run ``num_steps`` steps from ``u0`` and record the state after every ``record_every_steps`` of them: returns
    ``(ux, uy)`` stacked over the records on the dimension before the grid ((T, n, n), or (B, T, n, n) for a batch).
    The notebook's inner / outer loop without a host synchronisation per step; differentiable with respect to ``u0``."""
    if record_every_steps <= 0 or num_steps % record_every_steps:
        raise ValueError(f"num_steps = {num_steps} is not a positive multiple of record_every_steps = {record_every_steps}")
    u = _as_pair(u0)
    xs, ys = [], []
    for _ in range(num_steps // record_every_steps):
        u = equation(u, dt, steps=record_every_steps)
        xs.append(u[0])
        ys.append(u[1])
    return torch.stack(xs, dim=-3), torch.stack(ys, dim=-3)
