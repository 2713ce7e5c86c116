"""Shared pieces of the full-band (white-spectrum) tests of the fused spectral step, its tangent and its adjoint (test-only).

Inputs: half spectra of real WHITE fields (rms 5) and white complex cotangents, so that the de-aliasing cut, the Nyquist row and
column and every high-wavenumber twiddle carry energy -- the Gaussian spectra of the other derivative tests are zero to round-off
beyond |k| ~ 30.  From sample 1 on the zero and Nyquist columns get the non-Hermitian perturbation of
tests/test_ns2d_gpu.py::test_packed_nyquist_column_agrees_with_the_lone_tile (c2r semantics must drop those imaginary parts).

Measure: errors per spectral REGION of the (n, n//2+1) half spectrum -- the Nyquist row, the Nyquist and zero columns, the lines
just inside and just outside the 2/3-rule cut, the mean bin, the rest -- each as rms over the region of (got - ref), divided by
the rms of the WHOLE reference (where the mask zeroes the reference a region's own norm would be zero, or only the forcing
table's round-off).  A fault confined to one row or column cannot hide in a whole-field norm this way.

Reference: the CPU oracle (oracle/ns2d.py ``explicit_terms`` / ``advance``; for the IMEX schedules the stage loop of
tests/ns2d_ops.py, tied to the oracle by tests/test_ns2d_jvp_host.py) in fp64 from the (possibly fp32) inputs, under
torch.autograd.forward_ad for the tangents and torch.autograd.grad for the cotangents, on one host thread."""
import copy
import functools
import math

import torch

import ns2d_ops

L = 2 * math.pi
REAL = {"f64": torch.float64, "f32": torch.float32}
CPLX = {"f64": torch.complex128, "f32": torch.complex64}
IMEX = {"imex1": (1, 1.0, 1.0), "imex1.5": (1.5, 0.5, 0.5), "imex2": (2, 0.5, 0.5)}
# TCFD_NS2D_SIZES of csrc/tcfd_ns2d_plan.hpp: 2^k, 3 * 2^k and 5 * 2^k
FUSED_SIZES = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 96, 192, 384, 768, 80, 160, 320, 640, 1536, 1280)
REGION_NAMES = ("nyq_row", "nyq_col", "zero_col", "inside_cut", "outside_cut", "mean", "rest")


def dt_of(n):
    return 1e-3 if n <= 256 else 2.5e-4


def _white_fields(n, count, seed):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(count, n, n, generator=gen, dtype=torch.float64)
    return torch.fft.rfft2(5.0 * w / w.std())


@functools.lru_cache(maxsize=8)
def white_inputs(n, tag, B):
    """(w0, dw, g, g2) on the CPU in the precision of ``tag``: half spectra of two real white fields of rms 5 and two white
    complex cotangents; samples 1.. carry random imaginary parts in column 0 and a random complex offset in column n/2."""
    w0, dw = _white_fields(n, B, 6000 + n), _white_fields(n, B, 7000 + n)
    gen = torch.Generator().manual_seed(8000 + n + B)
    for x in (w0, dw):
        if B > 1:
            x[1:, :, 0] += 1j * 0.1 * torch.randn(B - 1, n, generator=gen, dtype=torch.float64) * x[1:, :, 0].abs().mean()
            x[1:, :, -1] += (0.05 + 0.1j) * torch.randn(B - 1, n, generator=gen, dtype=torch.float64) * x[1:, :, 1].abs().mean()
    g = torch.view_as_complex(torch.randn(B, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64))
    g2 = torch.view_as_complex(torch.randn(B, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64))
    return tuple(x.to(CPLX[tag]).contiguous() for x in (w0, dw, g, g2))


def dealias_extents(n):
    from torch_cfd_amd.spectral import dealias_extents as extents

    return extents(n)


@functools.lru_cache(maxsize=None)
def regions(n):
    """name -> boolean mask over the (n, n//2+1) half spectrum.  The lines cross (a row line meets every column line), and at
    n = 8 the first dropped column IS the Nyquist column: those bins belong to each of their lines.  "rest" is everything no
    line holds."""
    m = n // 2 + 1
    low, high, cols = dealias_extents(n)
    i, j = torch.arange(n)[:, None], torch.arange(m)[None, :]
    every = torch.ones(n, m, dtype=torch.bool)
    R = {"nyq_row": (i == n // 2) & every,
         "nyq_col": (j == n // 2) & every,
         "zero_col": (j == 0) & every,
         "inside_cut": ((i == low - 1) | (i == n - high) | (j == cols - 1)) & every,
         "outside_cut": ((i == low) | (i == n - high - 1) | (j == cols)) & every,
         "mean": (i == 0) & (j == 0)}
    held = torch.zeros(n, m, dtype=torch.bool)
    for mask in R.values():
        held |= mask
    R["rest"] = ~held
    return R


def kept(n):
    """The bins the 2/3-rule mask keeps, from ``dealias_extents``."""
    low, high, cols = dealias_extents(n)
    i, j = torch.arange(n)[:, None], torch.arange(n // 2 + 1)[None, :]
    return ((i < low) | (i >= n - high)) & (j < cols)


def region_errors(got, ref, scale_of=None):
    """{region: rms_R(got - ref) / rms_all(scale_of)} over every leading sample, plus "all" (the whole-field rel-L2 against
    ``scale_of``), "max_bin" (the largest single |got - ref| / rms_all(scale_of)) and "max_bin_at", its (sample, row, column).
    ``scale_of`` defaults to ``ref``; dw/dt passes ref_state / dt (what cancels in it, ``scaled_err`` of tests/test_ns2d_gpu.py)."""
    got, ref = (torch.as_tensor(x).detach().to("cpu", torch.complex128) for x in (got, ref))
    scale_of = ref if scale_of is None else torch.as_tensor(scale_of).detach().to("cpu", torch.complex128)
    n = ref.shape[-2]
    err2 = (got - ref).abs().pow(2).reshape(-1, n, n // 2 + 1)
    rms_all = scale_of.abs().pow(2).mean().sqrt().item()
    out = {}
    for name, mask in regions(n).items():
        out[name] = (err2[:, mask].mean().sqrt().item() / rms_all) if mask.any() else 0.0
    out["all"] = err2.mean().sqrt().item() / rms_all
    out["max_bin"] = err2.max().sqrt().item() / rms_all
    flat = int(err2.argmax())
    out["max_bin_at"] = (flat // (n * (n // 2 + 1)), flat // (n // 2 + 1) % n, flat % (n // 2 + 1))     # (sample, row, column)
    return out


def worst_region(errs):
    name = max(REGION_NAMES + ("all",), key=lambda k: errs[k])
    return name, errs[name]


def fmt(errs):
    return " ".join(f"{k}={errs[k]:.1e}" for k in REGION_NAMES + ("all", "max_bin")) + " at " + str(errs["max_bin_at"])


def jvp(fn, w, dw):
    """(primal outputs, tangent outputs) of a function returning one tensor or a tuple of tensors, by forward_ad."""
    import torch.autograd.forward_ad as fwAD

    with fwAD.dual_level():
        out = fn(fwAD.make_dual(w, dw))
        single = not isinstance(out, tuple)
        pairs = [fwAD.unpack_dual(o) for o in ((out,) if single else out)]
        prim, tang = [p.primal.detach().clone() for p in pairs], [p.tangent.detach().clone() for p in pairs]
    return (prim[0], tang[0]) if single else (prim, tang)


def oracle_functions(n, forcing, smooth, solver, dt, steps, real=torch.float64, mutate=None):
    """(explicit_terms(w), advance(w) -> (w_new, dwdt)) of the CPU oracle with tables in ``real``.  ``mutate(tables)`` edits a
    copy of the oracle's tables first (the host test's deliberately wrong tables)."""
    from oracle import ns2d as O

    t = ns2d_ops.tables(n, forcing, smooth, real=real)
    if mutate is not None:
        o = copy.copy(t.oracle)
        mutate(o)
        t = copy.copy(t)
        t.oracle, t.kx, t.ky = o, o.kx, o.ky
        t.mask = o.mask if smooth else None
    if solver == "rk4":
        return (lambda w: O.explicit_terms(w, t.oracle)), (lambda w: O.advance(w, dt, t.oracle, steps=steps))
    import torch_cfd_amd as tc

    old = torch.get_default_dtype()
    torch.set_default_dtype(real)
    try:
        order, alpha, beta = IMEX[solver]
        sched = ns2d_ops.schedule(tc.IMEXStepper(order=order, alpha=alpha, beta=beta), dt)
    finally:
        torch.set_default_dtype(old)

    def advance(w):
        new = ns2d_ops.advance(w, t, sched, steps)
        return new, 1 / (steps * dt) * (new - w)

    return (lambda w: ns2d_ops.explicit_terms(w, t)), advance


def evaluate(explicit, advance, w0, dw, g, g2, dt, steps, parts=("F", "step", "adjoint")):
    """Every quantity of the sweep from two functions of the state: F, dF; w, dwdt and the stepped tangent; wbar = J^T g and
    wbar2, the cotangent of  <g, w_new> + <g2 steps dt, dwdt>  (g2 scaled to weigh like g, as
    tests/test_ns2d_step_vjp_gpu.py::test_one_node_path_matches_the_per_stage_nodes)."""
    out = {}
    if "F" in parts:
        out["F"], out["dF"] = jvp(explicit, w0, dw)
    if "step" in parts:
        (out["w"], out["dwdt"]), (out["dw"], _) = jvp(advance, w0, dw)
    if "adjoint" in parts:
        w = w0.clone().requires_grad_(True)
        new, dwdt = advance(w)
        (out["wbar"],) = torch.autograd.grad(ns2d_ops.real_inner(g, new), w, retain_graph=True)
        (out["wbar2"],) = torch.autograd.grad(ns2d_ops.real_inner(g, new) + ns2d_ops.real_inner(g2 * (steps * dt), dwdt), w)
        if "w" not in out:
            out["w"], out["dwdt"] = new.detach(), dwdt.detach()
    return out


@functools.lru_cache(maxsize=8)
def reference(n, tag, B, forcing="kolmogorov", smooth=True, solver="rk4", steps=1, real=torch.float64):
    """``evaluate`` on the CPU oracle in ``real`` (fp64: the reference; fp32: the oracle's own single-precision run) from
    ``white_inputs(n, tag, B)``, on ONE host thread: multi-threaded MKL transforms of large complex64 arrays have returned
    wrong values on many-core hosts (tests/test_ns2d_gpu.py::test_against_oracle)."""
    cplx = torch.complex128 if real == torch.float64 else torch.complex64
    w0, dw, g, g2 = (x.to(cplx) for x in white_inputs(n, tag, B))
    dt = dt_of(n)
    threads, old = torch.get_num_threads(), torch.get_default_dtype()
    torch.set_num_threads(1)
    torch.set_default_dtype(real)
    try:
        explicit, advance = oracle_functions(n, forcing, smooth, solver, dt, steps, real)
        return evaluate(explicit, advance, w0, dw, g, g2, dt, steps)
    finally:
        torch.set_num_threads(threads)
        torch.set_default_dtype(old)
