"""Interpolation schemes of the finite-volume advection, under the names of torch_cfd/interpolation.py: ``linear``,
``upwind``, ``lax_wendroff``, ``van_leer_limiter`` and ``apply_tvd_limiter``.

In the reference these are Python functions on ``GridVariable``s that ``advect_general`` calls.  Here the advection runs
inside the HIP stage kernel (``csrc/tcfd_fvm.hip``), which has one instantiation per scheme, so the names are *descriptors*:
plain immutable objects that compare and hash by value and select an instantiation.  They are not callable and not
``nn.Module``s (an equation that holds one keeps its ``state_dict`` layout).  ``fvm.advection`` turns one into the ``convect``
argument of ``NavierStokes2DFVMProjection``::

    from torch_cfd_amd import fvm, interpolation
    eq = NavierStokes2DFVMProjection(nu, grid, convect=fvm.advection(interpolation.upwind), solver=...)

``apply_tvd_limiter(lax_wendroff, van_leer_limiter)`` is the reference's default (van Leer) and the only limited scheme it has;
any other combination raises ``NotImplementedError``.
"""
from __future__ import annotations

from dataclasses import dataclass

from . import _lib

__all__ = ["Interpolation", "Limiter", "linear", "upwind", "lax_wendroff", "van_leer_limiter", "apply_tvd_limiter"]


@dataclass(frozen=True)
class Interpolation:
    """An interpolation of a transported quantity to the faces of its control volume: its name in the reference and the
    ``TCFD_FVM_*`` scheme of the kernel that restates it."""

    name: str
    scheme: int

    def __repr__(self) -> str:
        return f"interpolation.{self.name}"


@dataclass(frozen=True)
class Limiter:
    """A flux limiter (the reference has one, ``van_leer_limiter``)."""

    name: str

    def __repr__(self) -> str:
        return f"interpolation.{self.name}"


linear = Interpolation("linear", _lib.TCFD_FVM_LINEAR)
upwind = Interpolation("upwind", _lib.TCFD_FVM_UPWIND)
lax_wendroff = Interpolation("lax_wendroff", _lib.TCFD_FVM_LAX_WENDROFF)
van_leer_limiter = Limiter("van_leer_limiter")

_VAN_LEER = Interpolation("apply_tvd_limiter(lax_wendroff, van_leer_limiter)", _lib.TCFD_FVM_VAN_LEER)


def apply_tvd_limiter(interpolation_fn: Interpolation, limiter: Limiter = van_leer_limiter) -> Interpolation:
    """The TVD combination of ``upwind`` and ``interpolation_fn`` weighted by ``limiter`` (interpolation.py:251).  The
    kernels hold the reference's one combination, ``(lax_wendroff, van_leer_limiter)``."""
    if interpolation_fn != lax_wendroff or limiter != van_leer_limiter:
        raise NotImplementedError(f"apply_tvd_limiter({interpolation_fn!r}, {limiter!r}): the finite-volume kernels implement "
                                  "apply_tvd_limiter(interpolation.lax_wendroff, interpolation.van_leer_limiter) only")
    return _VAN_LEER
