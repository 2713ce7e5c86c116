"""Plain-torch restatement of the finite-volume step (test-only): the same operation order as the HIP kernels and the
reference (torch_cfd/fvm.py, interpolation.py, finite_differences.py, pressure.py), on (..., n, n) tensors of any batch.
It lets GPU tests check sizes and batches no golden covers; tests/test_fvm_host.py checks it against the goldens."""
import math

import torch


def _sh(x, k, axis):
    """x.shift(k, axis): entry i holds x[i + k] (periodic)."""
    return torch.roll(x, -k, dims=axis)


def _half(a, b):
    return 0.5 * a + 0.5 * b


def _tvd_flux(cm, c0, c1, c2, w, cfl):
    pos = w > 0
    clow = torch.where(pos, c0, c1)
    cr = cfl * w
    d = c1 - c0
    hp = c0 + 0.5 * (1 - cr) * d
    hn = c1 - 0.5 * (1 + cr) * d
    chigh = torch.where(pos, hp, hn)
    dd = torch.where(d != 0, d, torch.ones_like(d))

    def lim(r):
        rp1 = 1 + r
        return torch.where(r > 0, (2 * r) / torch.where(rp1 != 0, rp1, torch.ones_like(rp1)), torch.zeros_like(r))

    phi = torch.where(pos, lim((c0 - cm) / dd), lim((c2 - c1) / dd))
    return (clow - (clow - chigh) * phi) * w


def _advect(c, wx, wy, cfl, h):
    ax, ay = -2, -1
    fx = _tvd_flux(_sh(c, -1, ax), c, _sh(c, 1, ax), _sh(c, 2, ax), wx, cfl)
    fy = _tvd_flux(_sh(c, -1, ay), c, _sh(c, 1, ay), _sh(c, 2, ay), wy, cfl)
    return -((fx - _sh(fx, -1, ax)) / h + (fy - _sh(fy, -1, ay)) / h)


def laplacian(u, h):
    s = 1 / h**2
    out = -2 * u * (s + s)
    out = out + (_sh(u, -1, -2) + _sh(u, 1, -2)) * s
    return out + (_sh(u, -1, -1) + _sh(u, 1, -1)) * s


def explicit_terms(ux, uy, dt, h, nu, drag=0.0, force=None):
    """du/dt of the staggered pair: van Leer advection + nu lap + force - drag u (force: (fx, fy) already / density)."""
    cfl = dt / h
    conv_x = _advect(ux, _half(ux, _sh(ux, 1, -2)), _half(uy, _sh(uy, 1, -2)), cfl, h)
    conv_y = _advect(uy, _half(ux, _sh(ux, 1, -1)), _half(uy, _sh(uy, 1, -1)), cfl, h)
    kx = conv_x + nu * laplacian(ux, h)
    ky = conv_y + nu * laplacian(uy, h)
    if force is not None:
        kx = kx + force[0]
        ky = ky + force[1]
    if drag > 0:
        kx = kx + ux * -drag
        ky = ky + uy * -drag
    return kx, ky


def inverse_eigenvalues(n, h, dtype=torch.float64):
    col = torch.zeros(n, dtype=dtype)
    col[0] = -2 / h**2
    col[1] = col[-1] = 1 / h**2
    lam = torch.fft.fft(col)[:, None] + torch.fft.rfft(col)[None, :]
    return torch.where(torch.abs(lam) > 10 * torch.finfo(torch.float32).eps, 1 / lam, 0)


def project(ux, uy, h, inverse):
    div = (ux - _sh(ux, -1, -2)) / h + (uy - _sh(uy, -1, -1)) / h
    q = torch.fft.irfft2(inverse * torch.fft.rfft2(div), s=div.shape[-2:])
    return ux - (_sh(q, 1, -2) - q) / h, uy - (_sh(q, 1, -1) - q) / h


def step(ux, uy, dt, a, b, h, nu, drag=0.0, force=None, inverse=None):
    """One RK step; a (stages x stages row-major) and b are the increments' weights dt * a_ij, dt * b_j (0: skipped)."""
    s = len(b)
    if inverse is None:
        inverse = inverse_eigenvalues(ux.shape[-1], h).to(ux.device)
    ks = []
    cur = (ux, uy)
    for i in range(s):
        if i > 0:
            px, py = ux, uy
            for j in range(i):
                if a[i * s + j] != 0:
                    px = px + a[i * s + j] * ks[j][0]
                    py = py + a[i * s + j] * ks[j][1]
            cur = project(px, py, h, inverse)
        ks.append(explicit_terms(cur[0], cur[1], dt, h, nu, drag, force))
    px, py = ux, uy
    for j in range(s):
        if b[j] != 0:
            px = px + b[j] * ks[j][0]
            py = py + b[j] * ks[j][1]
    return project(px, py, h, inverse)


def kolmogorov_staggered(n, wave, scale=1.0, L=2 * math.pi, dtype=torch.float64):
    """Kolmogorov forcing sampled at the staggered faces: fx = sin(k y) at y = (j + 1/2) h, fy = 0."""
    h = L / n
    y = (torch.arange(n, dtype=dtype) + 0.5) * h
    fx = scale * torch.sin(wave * (2 * math.pi / L) * y)[None, :].expand(n, n).contiguous()
    return fx, torch.zeros_like(fx)


# ---- inputs at the edges (tests/golden/make_golden_fvm.py edges() and the GPU tests at sizes no golden covers)
EDGE_STARTS = ("rest", "blocks", "checker", "integers")

# explicit tableaux beyond the named methods: two earlier stages feeding one stage state, negative weights, a zero row
TABLEAUX = {
    "rule38": {"a": [[1 / 3], [-1 / 3, 1.0], [1.0, -1.0, 1.0]], "b": [1 / 8, 3 / 8, 3 / 8, 1 / 8]},
    "ssprk3": {"a": [[1.0], [1 / 4, 1 / 4]], "b": [1 / 6, 1 / 6, 2 / 3]},
    "zero_row": {"a": [[0.0], [0.0, 1 / 2]], "b": [0.0, 0.0, 1.0]},
}


OPTIONAL_TERMS = ("plain", "dense", "negdrag")   # the a2_* groups of tests/golden/fvm_edges.npz


def degenerate_start(name, n, seed=0, dtype=torch.float64):
    """(2, n, n) velocity of small integers, so that the van Leer limiter's ties (face velocity w == 0, difference
    d == 0) are exact in any precision: rest; 4 x 4 blocks of {-1, 0, 1, 2}; a +-1 checkerboard (w == 0 on every face,
    d != 0); integers in [-2, 2]."""
    gen = torch.Generator().manual_seed(seed)
    if name == "rest":
        u = torch.zeros(2, n, n)
    elif name == "blocks":
        u = torch.randint(-1, 3, (2, n // 4, n // 4), generator=gen).repeat_interleave(4, -2).repeat_interleave(4, -1)
    elif name == "checker":
        i = torch.arange(n)
        sign = 1 - 2 * ((i[:, None] + i[None, :]) % 2)
        u = torch.stack([sign, -sign])
    elif name == "integers":
        u = torch.randint(-2, 3, (2, n, n), generator=gen)
    else:
        raise ValueError(name)
    return u.to(dtype)


def cotangent(shape, seed, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


class Physics:
    """One configuration of the solver, for the restatement and for the package alike: domain [0, length]^2, n x n."""

    def __init__(self, n, length=2 * math.pi, nu=1e-3, drag=0.1, density=1.0, wave=2):
        self.n, self.length, self.nu, self.drag, self.density, self.wave = n, length, nu, drag, density, wave   # wave None: unforced
        self.h = length / n

    @classmethod
    def of_golden(cls, g, group, n=None):
        """The physics of one group (``a1``, ``a2_plain``, ``a2_dense``, ``a3``) of tests/golden/fvm_edges.npz, at the
        golden's n or another."""
        n = int(g["n"]) if n is None else n
        if group.startswith("a2_"):
            return cls(n, float(g[f"{group}_length"]), float(g[f"{group}_nu"]), float(g[f"{group}_drag"]),
                       float(g[f"{group}_density"]), int(g["wave"]) if bool(g[f"{group}_forced"]) else None)
        return cls(n, 2 * math.pi, float(g["a1_nu"]), float(g["a1_drag"]), 1.0, int(g["wave"]))

    def tables(self, device="cpu", dtype=torch.float64):
        """(force / density, inverse eigenvalues): formed in fp64 and then rounded to `dtype`, as the package's plan does."""
        force = None
        if self.wave is not None:
            force = tuple((f / self.density).to(device, dtype) for f in kolmogorov_staggered(self.n, self.wave, L=self.length))
        inv = inverse_eigenvalues(self.n, self.h)
        return force, inv.to(device, torch.complex128 if dtype == torch.float64 else torch.complex64)

    def explicit(self, dt, device="cpu", dtype=torch.float64):
        force, _ = self.tables(device, dtype)
        return lambda u: explicit_terms(u[0], u[1], dt, self.h, self.nu / self.density, self.drag, force)

    def projection(self, device="cpu", dtype=torch.float64):
        _, inv = self.tables(device, dtype)
        return lambda u: project(u[0], u[1], self.h, inv)

    def rollout(self, a, b, dt, steps, device="cpu", dtype=torch.float64):
        force, inv = self.tables(device, dtype)

        def run(u):
            ux, uy = u
            for _ in range(steps):
                ux, uy = step(ux, uy, dt, a, b, self.h, self.nu / self.density, self.drag, force, inv)
            return ux, uy
        return run

    def grid(self):
        import torch_cfd_amd as tc

        return tc.Grid(shape=(self.n, self.n), domain=((0, self.length), (0, self.length)))

    def equation(self, solver=None):
        """The package's equation of this configuration."""
        import torch_cfd_amd as tc

        grid = self.grid()
        forcing = None
        if self.wave is not None:
            forcing = tc.KolmogorovForcing(grid=grid, diam=self.length, wave_number=self.wave, offsets=grid.cell_faces)
        return tc.NavierStokes2DFVMProjection(self.nu, grid, drag=self.drag, density=self.density, forcing=forcing, solver=solver)
