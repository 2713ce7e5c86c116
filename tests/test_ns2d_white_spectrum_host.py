"""Host-side checks of the white-spectrum sweep (no GPU): what tests/test_ns2d_white_spectrum_gpu.py measures has teeth.

1. Four deliberately wrong tables of the CPU oracle -- one extra kept row of the 2/3-rule mask, one extra kept column, the sign
   of kx on the Nyquist row, kx of one row off by 1 % -- are each put above the sweep's bounds by ``region_errors`` under
   ``white_inputs``, in the region that names the fault.
2. The same wrong tables under the smooth inputs of tests/test_ns2d_jvp_gpu.py change dF and the stepped tangent by less than
   1e-12: the blind spot the sweep closes.  (A regression note: whoever feeds those tests full-band data deletes this check.)
3. The fp32 bounds of the sweep are reachable: the oracle in complex64 against itself in complex128 stays inside them in every
   region of every quantity.
4. ``regions(n)`` covers the half spectrum, its lines are those of ``brick_wall_filter_2d`` at every fused size.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ns2d_white_ops as W  # noqa: E402

L = 2 * math.pi
F64_BOUND = {"F": 1e-10, "dF": 1e-10, "dw": 1e-9, "wbar": 1e-9}
F32_BOUND = {"F": 2e-5, "dF": 2e-5, "w": 4e-6, "dwdt": 4e-6, "dw": 2e-5, "wbar": 2e-5, "wbar2": 2e-5}
LINES = ("nyq_row", "nyq_col", "zero_col", "inside_cut", "outside_cut")


def _mutants(n):
    """name -> edit of a copy of the oracle's tables."""
    low, high, cols = W.dealias_extents(n)
    row = round(100 * n / 256)          # a row in the band the mask removes: it still feeds the physical-space product

    def extra_row(t):
        t.mask = t.mask.clone()
        t.mask[low, :cols] = 1

    def extra_col(t):
        t.mask = t.mask.clone()
        t.mask[:low, cols] = 1
        t.mask[n - high:, cols] = 1

    def nyq_kx_sign(t):
        t.kx = t.kx.clone()
        t.kx[n // 2, :] = -t.kx[n // 2, :]

    def kx_row_1pct(t):
        t.kx = t.kx.clone()
        t.kx[row, :] = t.kx[row, :] * 1.01

    return {"extra_row": extra_row, "extra_col": extra_col, "nyq_kx_sign": nyq_kx_sign, "kx_row_1pct": kx_row_1pct}


def _run(n, mutate, w0, dw, g, g2):
    torch.set_default_dtype(torch.float64)
    dt = W.dt_of(n)
    explicit, advance = W.oracle_functions(n, "kolmogorov", True, "rk4", dt, 1, mutate=mutate)
    return W.evaluate(explicit, advance, w0, dw, g, g2, dt, 1)


@pytest.mark.parametrize("n", [64, 256])
def test_the_measure_catches_wrong_tables_under_white_inputs(n):
    w0, dw, g, g2 = W.white_inputs(n, "f64", 1)
    clean = _run(n, None, w0, dw, g, g2)
    for name, mutate in _mutants(n).items():
        wrong = _run(n, mutate, w0, dw, g, g2)
        errs = {q: W.region_errors(wrong[q], clean[q]) for q in ("F", "dF", "dw", "wbar")}
        for q, e in errs.items():
            print(f"n={n} {name} {q}: {W.fmt(e)}")
        for q in ("F", "dF"):
            assert W.worst_region(errs[q])[1] > F32_BOUND[q], (name, q)
        for q in ("dw", "wbar"):
            assert W.worst_region(errs[q])[1] > (F64_BOUND[q] if name == "kx_row_1pct" else F32_BOUND[q]), (name, q)
        if name in ("extra_row", "extra_col"):
            # the line the mask wrongly keeps: the reference is zero (F, dF) or untouched by F (the stepped tangent) there
            for q in ("F", "dF", "dw"):
                assert errs[q]["outside_cut"] > F32_BOUND[q], (name, q)
                assert errs[q]["outside_cut"] > 3 * errs[q]["rest"], (name, q)
            assert max(errs["wbar"][r] for r in LINES) > F32_BOUND["wbar"], name
        elif name == "nyq_kx_sign":
            # F and the tangents see the row through the physical-space product (every kept bin moves, the lines included);
            # the cotangent of the row itself is the transposed derivative: the Nyquist row of wbar stands out
            for q in ("F", "dF", "dw", "wbar"):
                assert max(errs[q][r] for r in LINES) > F32_BOUND[q], (name, q)
            assert errs["wbar"]["nyq_row"] > 3 * errs["wbar"]["rest"], name
        else:
            for q in ("F", "dF"):
                assert errs[q]["rest"] > F32_BOUND[q] and errs[q]["all"] > F32_BOUND[q], (name, q)
            for q in ("dw", "wbar"):
                assert errs[q]["rest"] > F64_BOUND[q] and errs[q]["all"] > F64_BOUND[q], (name, q)


def test_the_smooth_inputs_of_the_tangent_tests_do_not_see_them():
    """n = 256 (at n = 64 the Gaussian envelopes still reach the cut: exp(-21^2 / 72) = 2e-3).  If this fails because
    tests/test_ns2d_jvp_gpu.py::inputs became full-band, delete it."""
    import test_ns2d_jvp_gpu as J

    n = 256
    w0, dw = J.inputs(n, "f64", 1)
    _, _, g, g2 = W.white_inputs(n, "f64", 1)
    clean = _run(n, None, w0, dw, g, g2)
    for name, mutate in _mutants(n).items():
        wrong = _run(n, mutate, w0, dw, g, g2)
        for q in ("dF", "dw"):
            e = W.region_errors(wrong[q], clean[q])
            print(f"n={n} smooth inputs, {name} {q}: {W.fmt(e)}")
            assert W.worst_region(e)[1] < 1e-12, (name, q)


@pytest.mark.parametrize("n", [8, 80, 96, 1280])
def test_the_fp32_bounds_are_reachable(n):
    """The oracle in complex64 against the oracle in complex128, from the same complex64 inputs."""
    ref = W.reference(n, "f32", 2)
    own = W.reference(n, "f32", 2, real=torch.float32)
    total = W.dt_of(n)
    for q, bound in F32_BOUND.items():
        assert own[q].dtype == torch.complex64
        e = W.region_errors(own[q], ref[q], ref["w"] / total if q == "dwdt" else None)
        print(f"n={n} {q}: {W.fmt(e)}")
        assert W.worst_region(e)[1] <= bound, (q, W.worst_region(e))
    if n == 1280:
        W.reference.cache_clear()


@pytest.mark.parametrize("n", W.FUSED_SIZES)
def test_regions_cover_the_half_spectrum_along_the_lines_of_the_filter(n):
    import torch_cfd_amd as tc
    from oracle import ns2d as O

    m = n // 2 + 1
    low, high, cols = W.dealias_extents(n)
    if n == 128:
        assert (low, high) == (42, 43)
    R = W.regions(n)
    assert tuple(R) == W.REGION_NAMES and all(v.shape == (n, m) and v.dtype == torch.bool for v in R.values())
    count = sum(v.to(torch.int64) for v in R.values())
    assert bool((count >= 1).all())
    # "rest" is exactly what lies on no line, counted once; a bin counted more than once sits where a row line crosses a
    # column line -- or, at n = 8 only, where two lines coincide (the first dropped row is the Nyquist row, the first dropped
    # column the Nyquist column) -- or is the mean bin (on the zero column)
    row_lines, col_lines = [n // 2, low - 1, n - high, low, n - high - 1], [n // 2, 0, cols - 1, cols]
    if n > 8:
        assert len(set(row_lines)) == 5 and len(set(col_lines)) == 4
    on_row, on_col = torch.zeros(n, dtype=torch.bool), torch.zeros(m, dtype=torch.bool)
    on_row[row_lines], on_col[col_lines] = True, True
    assert torch.equal(R["rest"], ~on_row[:, None] & ~on_col[None, :])
    assert bool((count[R["rest"]] == 1).all())
    crossing = on_row[:, None] & on_col[None, :]
    many = count > 1
    if n > 8:
        assert bool((many <= (crossing | R["mean"])).all())
    assert R["mean"].sum() == 1 and bool(R["mean"][0, 0]) and bool(R["zero_col"][0, 0])
    assert R["nyq_row"].sum() == m and R["nyq_col"].sum() == n and R["zero_col"].sum() == n
    # the lines are the filter's: last kept and first dropped
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        mask = tc.brick_wall_filter_2d(tc.Grid(shape=(n, n), domain=((0, L), (0, L)))).bool()
    finally:
        torch.set_default_dtype(old)
    assert torch.equal(mask, O.brick_wall_mask(n).bool()) and torch.equal(mask, W.kept(n))
    assert bool(mask[low - 1, :cols].all()) and bool(mask[n - high, :cols].all()) and not bool(mask[low].any())
    assert not bool(mask[n - high - 1].any()) and not bool(mask[:, cols].any())
    assert bool(mask[:low, cols - 1].all()) and bool(mask[n - high:, cols - 1].all())
    # "outside_cut" holds no kept bin; "inside_cut" holds the two last kept rows and the last kept column (two shared corners)
    assert not bool((mask & R["outside_cut"]).any())
    assert int((mask & R["inside_cut"]).sum()) == 2 * cols + (low + high) - 2
