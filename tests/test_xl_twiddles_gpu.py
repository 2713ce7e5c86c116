"""GPU: the cross-lane column transforms with table twiddles in their second stage and the plane pass with folded constants,
at the smallest shapes where those code paths run, and the 1024-point cross-lane row transform beside them.

* the 1024-point transform alone (tcfd_debug_xl_fft1024), both directions, against numpy through the map of its output
  permutation -- checked as tests/micro/xl_fft_check.py checks it: max |error| <= 1e-12 max |reference|;
* one and five forward(w, dt) calls at n = 1024, fp64, B = 1 and B = 3 (an odd count: the invalid-pair tail of the persistent
  row grid and a partial chunk), Kolmogorov forcing and drag as in bench.py, against oracle/ns2d.py on the host: split
  columns, packed Nyquist column, MODE_A / CA / C.  Bounds of DESIGN section 2: 1e-10 (rel-L2) on the state and on dw/dt;
* the same at n = 512, B = 2 (the non-split 512-point column tile);
* n = 1024, B = 1, fp32, one step: 2e-6 on the state, and on dw/dt measured against what cancels (scaled_err, as
  tests/test_ns2d_gpu.py does); the fp32 instantiations keep the squaring chains: they still build and agree.

The fields of a batch evolve independently, so the oracle runs once per size on the largest batch and every case reads its
slice.  Measured (fp64): state 4e-17 after one step, 1.8e-16 after five, dw/dt 1.5e-14 ... 3.2e-14; transform alone 5e-16."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

L = 2 * math.pi
DT = {1024: 6.136e-4, 512: 1e-3}
REAL = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def scaled_err(a, b, scale_of):
    a, b, s = (torch.as_tensor(x).to("cpu", torch.complex128) for x in (a, b, scale_of))
    return (torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(s.reshape(-1))).item()


def build_op(n, tag, dev):
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False)
    return tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, smooth=True, forcing_fn=forcing,
                                     solver=tc.RK4CrankNicolsonStepper()).to(dev)


_REF = {}


def reference(n, tag, B, steps):
    """(w0, {k: (w_k, dw/dt of call k, w_{k-1})}) of `steps` successive oracle calls on B fields; computed once per (n, tag)."""
    from oracle import ns2d as O

    key = (n, tag)
    if key not in _REF:
        real = REAL[tag]
        t = O.make_tables(n, L, 1e-3, 0.1, True, None, real)
        t.forcing_hat = O.kolmogorov_forcing_hat(n, L, t.kx, t.ky, 1.0, 4, False, False, real=real)
        w0 = torch.stack([torch.fft.rfft2(O.mcwilliams_vorticity(n, L, 4, s, real)) for s in range(B)])
        out, w = {}, w0
        for k in range(1, steps + 1):
            wn, d = O.advance(w, DT[n], t)
            out[k] = (wn, d)
            w = wn
        _REF[key] = (w0, out)
    w0, out = _REF[key]
    assert w0.shape[0] >= B and max(out) >= steps
    return w0, out


def kmap():
    """output index held by register t of lane j after the natural -> pi transform (tcfd_fft.hpp, xl_fft1024)"""
    K = np.zeros((8, 128), dtype=int)
    for t in range(8):
        for j in range(128):
            w, l = j >> 6, j & 63
            lb = lambda b: (l >> b) & 1
            K[t, j] = ((w << 2) | (lb(1) << 1) | lb(0)) + 8 * ((lb(5) << 2) | (lb(4) << 1) | (t & 1)) \
                + 64 * ((lb(3) << 1) | lb(2)) + 256 * ((((t >> 2) & 1) << 1) | ((t >> 1) & 1))
    return K.reshape(-1)


def test_xl_fft1024_both_directions(dev):
    import torch_cfd_amd as tc

    plan = tc.fft_plan(1024, torch.complex128, dev)
    lib = tc._lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(7)
    S = 6
    z = rng.standard_normal((S, 1024)) + 1j * rng.standard_normal((S, 1024))
    z[S - 1] = 0
    z[S - 1, 333] = 1.0    # unit impulse at an odd index: every output is a single root of unity
    K = kmap()
    # dir = +1: natural order in, exp(+) transform out in the permutation pi
    zin = torch.from_numpy(z).to(dev)
    out = torch.empty_like(zin)
    tc._lib.check(lib.tcfd_debug_xl_fft1024(plan.handle, zin.data_ptr(), out.data_ptr(), S, 1, st), "xl +1")
    torch.cuda.synchronize()
    got = np.zeros_like(z)
    got[:, K] = out.cpu().numpy()
    ref = np.fft.ifft(z, axis=-1) * 1024
    for s in range(S):
        err = np.abs(got[s] - ref[s]).max() / np.abs(ref[s]).max()
        print(f"dir +1 row {s}: max err / max |ref| = {err:.3e}")
        assert err <= 1e-12
    # dir = -1: input in the permutation pi, exp(-) transform out in natural order
    pin = np.ascontiguousarray(z[:, K])
    tin = torch.from_numpy(pin).to(dev)
    tc._lib.check(lib.tcfd_debug_xl_fft1024(plan.handle, tin.data_ptr(), out.data_ptr(), S, -1, st), "xl -1")
    torch.cuda.synchronize()
    f = out.cpu().numpy()
    reff = np.fft.fft(z, axis=-1)
    for s in range(S):
        err = np.abs(f[s] - reff[s]).max() / np.abs(reff[s]).max()
        print(f"dir -1 row {s}: max err / max |ref| = {err:.3e}")
        assert err <= 1e-12


def run_case(n, tag, B, steps, tol, dev):
    w0, ref = reference(n, tag, {1024: 3, 512: 2}[n] if tag == "f64" else 1, 5 if tag == "f64" else 1)
    op = build_op(n, tag, dev)
    dt = DT[n]
    w = w0[:B].to(dev)
    d = None
    for _ in range(steps):
        w, d = op(w, dt)
    wr, dr = ref[steps]
    e_w = rel_l2(w, wr[:B])
    e_d = scaled_err(d, dr[:B], wr[:B] / dt)
    print(f"n={n} {tag} B={B} steps={steps}: state rel-L2 {e_w:.3e}, dw/dt scaled {e_d:.3e}, dw/dt rel-L2 {rel_l2(d, dr[:B]):.3e}")
    assert w.dtype == w0.dtype and torch.isfinite(torch.view_as_real(w)).all()
    assert e_w < tol
    if tag == "f64":
        assert rel_l2(d, dr[:B]) < tol    # dw/dt itself: the explicit terms, not the state error again
    else:
        assert e_d < tol                  # fp32: against what cancels


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("steps", [1, 5])
def test_1024_f64_steps_against_oracle(B, steps, dev):
    run_case(1024, "f64", B, steps, 1e-10, dev)


@pytest.mark.parametrize("steps", [1, 5])
def test_512_f64_steps_against_oracle(steps, dev):
    run_case(512, "f64", 2, steps, 1e-10, dev)


def test_1024_f32_one_step_against_oracle(dev):
    run_case(1024, "f32", 1, 1, 2e-6, dev)
