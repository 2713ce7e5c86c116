"""Plain-torch restatement of the finite-volume step with each advection scheme (test-only): tests/fvm_ops.py with its face
flux swapped for the two-cell fluxes of torch_cfd/interpolation.py (upwind :102, linear :39 / :71, lax_wendroff :171), in
the reference's operation order.  tests/test_fvm_schemes_host.py checks it against the reference's goldens at n = 16, which
licenses it as the yardstick of the GPU tests at the sizes and batches no golden covers."""
import contextlib

import torch

import fvm_ops as F
from fvm_ops import _half, _sh, laplacian, project, step  # noqa: F401  (laplacian, project: the parts the swap leaves alone)

SCHEMES = ("upwind", "linear", "lax_wendroff", "van_leer")


def _upwind_flux(c0, c1, w, cfl):
    return torch.where(w > 0, c0, c1) * w


def _linear_flux(c0, c1, w, cfl):
    return _half(c0, c1) * w


def _lax_wendroff_flux(c0, c1, w, cfl):
    cr = cfl * w
    d = c1 - c0
    hp = c0 + 0.5 * (1 - cr) * d
    hn = c1 - 0.5 * (1 + cr) * d
    return torch.where(w > 0, hp, hn) * w


FLUXES = {"upwind": _upwind_flux, "linear": _linear_flux, "lax_wendroff": _lax_wendroff_flux}


@contextlib.contextmanager
def _swapped(scheme):
    """fvm_ops with the flux of `scheme` in place of the van Leer flux (van_leer: as it is).  The swap holds only while the
    block runs: a closure that calls fvm_ops later must enter `_swapped` itself, inside its body, as `Physics.explicit` and
    `Physics.rollout` do -- one built inside the block and called after it would run van Leer."""
    if scheme == "van_leer":
        yield
        return
    flux, saved = FLUXES[scheme], F._tvd_flux
    F._tvd_flux = lambda cm, c0, c1, c2, w, cfl: flux(c0, c1, w, cfl)
    try:
        yield
    finally:
        F._tvd_flux = saved


def explicit_terms(scheme, ux, uy, dt, h, nu, drag=0.0, force=None):
    with _swapped(scheme):
        return F.explicit_terms(ux, uy, dt, h, nu, drag, force)


def convect(scheme, ux, uy, dt, h):
    """The advection term alone: the explicit terms without viscosity, drag and forcing."""
    return explicit_terms(scheme, ux, uy, dt, h, 0.0)


class Physics(F.Physics):
    """fvm_ops.Physics with an advection scheme, for the restatement and for the package alike."""

    def __init__(self, scheme, n, **kw):
        super().__init__(n, **kw)
        self.scheme = scheme

    def explicit(self, dt, device="cpu", dtype=torch.float64):
        force, _ = self.tables(device, dtype)
        return lambda u: explicit_terms(self.scheme, u[0], u[1], dt, self.h, self.nu / self.density, self.drag, force)

    def convect(self, dt):
        return lambda u: convect(self.scheme, u[0], u[1], dt, self.h)

    def rollout(self, a, b, dt, steps, device="cpu", dtype=torch.float64):
        force, inv = self.tables(device, dtype)

        def run(u):
            ux, uy = u
            with _swapped(self.scheme):
                for _ in range(steps):
                    ux, uy = step(ux, uy, dt, a, b, self.h, self.nu / self.density, self.drag, force, inv)
            return ux, uy
        return run

    def descriptor(self):
        """The package's `convect` argument of this scheme (van_leer: built explicitly through apply_tvd_limiter)."""
        from torch_cfd_amd import fvm, interpolation as I

        c = {"upwind": I.upwind, "linear": I.linear, "lax_wendroff": I.lax_wendroff,
             "van_leer": I.apply_tvd_limiter(I.lax_wendroff, I.van_leer_limiter)}[self.scheme]
        return fvm.advection(c)

    def equation(self, solver=None):
        import torch_cfd_amd as tc

        grid = self.grid()
        forcing = None
        if self.wave is not None:
            forcing = tc.KolmogorovForcing(grid=grid, diam=self.length, wave_number=self.wave, offsets=grid.cell_faces)
        return tc.NavierStokes2DFVMProjection(self.nu, grid, drag=self.drag, density=self.density, forcing=forcing, solver=solver,
                                              convect=self.descriptor())
