"""The fused spectral step, its tangent and its adjoint on FULL-BAND spectra, at every fused grid size in both precisions.

Every ``Cfg<T, N>`` of csrc/tcfd_ns2d_sized.hip (20 sizes x 2 precisions) runs the explicit terms, their tangent, the step (state
and dw/dt), the tangent-linear step, the adjoint model (``adjoint_step`` with and without ``g_dwdt``) and the per-stage autograd
nodes (TCFD_FUSED_ADJOINT=0) on white inputs (tests/ns2d_white_ops.py) against the CPU oracle in fp64 under forward_ad /
autograd.grad.  Errors are taken per spectral region (Nyquist row, Nyquist and zero columns, the lines on both sides of the
2/3-rule cut, the mean bin, the rest) over the rms of the whole reference, and over the whole field; tests/
test_ns2d_white_spectrum_host.py shows on the CPU that this measure catches one wrong mask line, a wrong sign on the Nyquist row
and a 1 % wavenumber error in one row, none of which the smooth inputs of the other derivative tests can see.

Bounds, the project's own (tests/test_ns2d_gpu.py::test_against_oracle, tests/test_ns2d_jvp_gpu.py,
tests/test_ns2d_step_vjp_gpu.py), on every region and on the whole field:
  fp64  F, dF, state, dw/dt scaled by |w| / dt: 1e-10; stepped tangents and gradients: 1e-9; the primal of tangent_step /
        adjoint_step against the plain step: 1e-12; the largest single bin under the bound of its quantity
  fp32  state and scaled dw/dt 4e-6, everything else 2e-5; the largest single bin is printed only (at the Kolmogorov bins the
        fp32 oracle itself is off by 1e-3 of the field's rms, the forcing table's round-off)
  the adjoint identity <J dw, g> = <dw, J^T g> with the white dw: 1e-12 / 1e-5 of |J dw| |g|
  F and dF are exactly zero on every bin the mask removes (F: apart from the forcing's own bins)

Measured on an MI355X: the worst region-or-whole-field value over the sizes of a family (after the slash, fp64 only: the largest
single bin); "w" stands for the scaled dw/dt too (the same figures), "wbar" for adjoint_step and the per-stage nodes alike
(they agree to the digits shown), "primal" for tangent_step's state against the plain step (adjoint_step's is bit-equal, 0).
                      F                  dF                 w                  tangent            wbar               wbar, g_dwdt   primal   identity
  fp64 2^k   8..4096  2.7e-14 / 2.3e-11  2.4e-15 / 1.3e-14  1.4e-16 / 3.2e-14  9.4e-17 / 1.9e-15  2.8e-16 / 3.8e-15  4.0e-16        1.1e-16  2.7e-17
       3*2^k 96..1536 9.9e-15 / 2.7e-12  3.1e-15 / 8.6e-15  7.8e-17 / 2.9e-15  5.5e-17 / 1.1e-15  2.3e-16 / 3.5e-15  3.4e-16        6.6e-17  8.0e-19
       5*2^k 80..1280 9.7e-15 / 2.8e-12  1.9e-15 / 6.9e-15  5.0e-17 / 2.9e-15  4.9e-17 / 9.1e-16  2.3e-16 / 2.0e-15  3.2e-16        4.3e-17  3.0e-18
       unmasked       1.6e-15 / 6.8e-15  1.6e-15 / 6.7e-15  6.0e-17 / 7.4e-16  6.1e-17 / 7.4e-16  2.3e-16 / 1.6e-15  3.3e-16        4.3e-17  1.9e-18
       IMEX           1.8e-15 / 2.2e-14  1.4e-15 / 4.8e-15  8.1e-17 / 5.3e-16  3.6e-17 / 3.6e-16  2.0e-16 / 9.5e-16  2.8e-16        8.1e-17  5.7e-18
  fp32 2^k            1.1e-06            1.1e-06            2.7e-07            3.9e-07            2.9e-07            3.2e-07        6.8e-08  1.2e-08
       3*2^k          1.0e-06            7.2e-07            1.3e-07            1.4e-07            1.7e-07            3.4e-07        3.4e-08  9.3e-10
       5*2^k          9.6e-07            6.9e-07            1.6e-07            1.5e-07            1.4e-07            2.5e-07        2.8e-08  1.1e-09
       unmasked       4.7e-07            4.3e-07            1.5e-07            1.5e-07            1.3e-07            2.0e-07        2.6e-08  5.3e-10
       IMEX           6.3e-07            5.5e-07            1.7e-07            1.0e-07            1.1e-07            1.7e-07        1.1e-08  1.4e-09
No region stands out at any size: a line region is at most 2.3 times its quantity's whole-field value (5.1 times in one figure
of 8e-17, the Nyquist row of tangent_step's state against the plain step at n = 64), the single mean bin at most 3.1 times.  The
one figure that grows with the grid is the largest single bin of the fp64 F, 1.9e-15 at n = 8 to 2.3e-11 at 4096 (whole field
6e-16 to 2.7e-14).  From n = 32 on it sits in row 0 at a column the mask removes (n = 64: column 28 of 22 kept; 4096: 1493 of
1366): the kernel's value there is an exact zero (asserted), the oracle's is the round-off of its forcing table -- rfft2 of
sin(4 y), constant along x, leaves its transform noise in row 0, and the curl multiplies it by ky.  It is the reference's own
error, a factor of four inside the bound at the largest size.  The fp32 single-bin values reach 1.3e-4 in F (the same table in
fp32, see above) and 5e-6 elsewhere.  n = 8 under the sweep's forcing runs unpruned (see ``_sweep``).
"""
import pytest
import torch

import ns2d_ops
import ns2d_step_vjp_ops as V
import ns2d_white_ops as W

pytestmark = pytest.mark.gpu

# bound per quantity: (fp64, fp32)
TOL = {"F": (1e-10, 2e-5), "F (jvp call)": (1e-10, 2e-5), "dF": (1e-10, 2e-5), "w": (1e-10, 4e-6), "dwdt (scaled)": (1e-10, 4e-6),
       "tangent": (1e-9, 2e-5), "wbar adjoint_step": (1e-9, 2e-5), "wbar per-stage nodes": (1e-9, 2e-5),
       "wbar adjoint_step g_dwdt": (1e-9, 2e-5), "wbar per-stage nodes g_dwdt": (1e-9, 2e-5),
       "tangent_step primal vs step": (1e-12, 2e-5), "adjoint_step primal vs step": (1e-12, 2e-5)}


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _sweep(n, tag, B, dev, monkeypatch, forcing="kolmogorov", smooth=True, solver="rk4", steps=1):
    ref = W.reference(n, tag, B, forcing, smooth, solver, steps)
    w0, dw, g, g2 = (x.to(dev) for x in W.white_inputs(n, tag, B))
    op = V.build_op(n, tag, forcing, dev, smooth, solver)
    info = op._plan(w0).info()
    assert "composite" not in info, info
    # wave number 4 is the Nyquist mode of an 8-point grid: sin(4 y) samples to round-off there, in every bin, nothing of it
    # stands out for ``forcing_noise_floor`` to keep, and the plan carries it as a dense table on the unpruned kernels
    degenerate = n == 8 and forcing == "kolmogorov"
    assert (info["keep_cols"] > 0) == (smooth and not degenerate), info
    dt = W.dt_of(n)
    total = steps * dt
    g2s = g2 * total                 # the cotangent of dwdt = (w_new - w) / (steps dt), scaled to weigh like g

    F = op.explicit_terms(w0)
    F2, dF = op.explicit_terms_jvp(w0, dw)
    w1, dwdt = op(w0, dt, steps)
    wt, dwt = op.tangent_step(w0, dw, dt, steps)
    wa, wbar = op.adjoint_step(w0, g, dt, steps)
    _, wbar2 = op.adjoint_step(w0, g, dt, steps, g_dwdt=g2s)
    monkeypatch.setenv("TCFD_FUSED_ADJOINT", "0")
    nodes, name = V.grad_through_forward(op, w0, dt, steps, g)
    nodes2, name2 = V.grad_through_forward(op, w0, dt, steps, g, g2s)
    monkeypatch.delenv("TCFD_FUSED_ADJOINT")
    assert "FusedSteps" not in name and "FusedSteps" not in name2, (name, name2)

    cases = [("F", F, ref["F"], None), ("F (jvp call)", F2, ref["F"], None), ("dF", dF, ref["dF"], None),
             ("w", w1, ref["w"], None), ("dwdt (scaled)", dwdt, ref["dwdt"], ref["w"] / total),
             ("tangent", dwt, ref["dw"], None), ("wbar adjoint_step", wbar, ref["wbar"], None),
             ("wbar per-stage nodes", nodes, ref["wbar"], None), ("wbar adjoint_step g_dwdt", wbar2, ref["wbar2"], None),
             ("wbar per-stage nodes g_dwdt", nodes2, ref["wbar2"], None),
             ("tangent_step primal vs step", wt, w1, None), ("adjoint_step primal vs step", wa, w1, None)]
    what = f"n={n} {tag} B={B} {forcing} smooth={smooth} {solver} steps={steps}"
    failures, summary = [], []
    for quantity, got, want, scale_of in cases:
        errs = W.region_errors(got, want, scale_of)
        print(f"{what} | {quantity}: {W.fmt(errs)}")
        bound = TOL[quantity][0 if tag == "f64" else 1]
        where, worst = W.worst_region(errs)
        summary.append(f"{quantity} {worst:.1e}@{where}")
        if worst > bound:
            failures.append((quantity, where, worst, bound))
        if tag == "f64" and errs["max_bin"] > bound:
            failures.append((quantity, "max_bin", errs["max_bin"], bound))
    lhs, rhs = ns2d_ops.real_inner(dwt, g).item(), ns2d_ops.real_inner(dw, wbar).item()
    scale = (torch.linalg.norm(dwt) * torch.linalg.norm(g)).item()
    defect = abs(lhs - rhs) / scale
    print(f"{what} | identity: <Jdw,g> {lhs:.12e} <dw,JTg> {rhs:.12e} defect/scale {defect:.3e}")
    print(f"{what} | WORST " + "; ".join(summary) + f"; identity {defect:.1e}")
    if defect > (1e-12 if tag == "f64" else 1e-5):
        failures.append(("identity", "", defect, 1e-12 if tag == "f64" else 1e-5))
    if smooth:
        removed = ~W.kept(n).to(dev)
        fh = op.forcing_hat()
        unforced = removed if fh is None else removed & (fh == 0).to(dev)
        for quantity, x, mask in (("F", F, unforced), ("F (jvp call)", F2, unforced), ("dF", dF, removed)):
            if not bool((x[..., mask] == 0).all()):
                failures.append((quantity, "a bin the mask removes is not exactly zero", x[..., mask].abs().max().item(), 0.0))
    assert not failures, (what, failures)


def _release(n):
    if n >= 1024:     # the large references (autograd graphs of 2048^2 / 4096^2 fields on the host) do not outlive the case
        W.reference.cache_clear()
        W.white_inputs.cache_clear()
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- (a) every instantiation
def test_the_size_list_is_the_set_of_fused_plans(dev):
    """FUSED_SIZES (TCFD_NS2D_SIZES spelled out: the library does not expose it) is exactly the set of grids whose plan is a
    library plan, among every 2^k, 3 * 2^k, 5 * 2^k and 7 * 2^k in 8..4096: the others report a composite or dense path."""
    from torch_cfd_amd.equations import _HipPlan

    candidates = sorted({p << k for p in (1, 3, 5, 7) for k in range(1, 13) if 8 <= p << k <= 4096})
    fused = set()
    for n in candidates:
        op = V.build_op(n, "f32", "none", dev)
        plan = op._plan(torch.zeros(1, n, n // 2 + 1, dtype=torch.complex64, device=dev))
        info = plan.info()
        if isinstance(plan, _HipPlan):
            assert "composite" not in info and "dense_dft" not in info, (n, info)
            fused.add(n)
        else:
            assert "composite" in info and (info["composite"] > 0 or info["dense_dft"] == 1), (n, info)
        del op, plan
    torch.cuda.empty_cache()
    assert fused == set(W.FUSED_SIZES) and len(W.FUSED_SIZES) == 20


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("n", [n for n in W.FUSED_SIZES if n != 4096])
def test_every_size_on_white_spectra(n, tag, dev, monkeypatch):
    """Kolmogorov forcing, drag 0.1, smooth=True, RK4-CN, one step at dt_of(n); B = 2 (sample 1 with non-Hermitian zero and
    Nyquist columns), B = 1 at 2048."""
    try:
        _sweep(n, tag, 1 if n >= 2048 else 2, dev, monkeypatch)
    finally:
        _release(n)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_the_pruned_plan_of_the_smallest_size(tag, dev, monkeypatch):
    """n = 8 without a forcing: under the Kolmogorov forcing of the sweep (the Nyquist mode of this grid, see ``_sweep``) the
    size runs unpruned; its pruned plan, with the packed Nyquist column, meets the oracle here."""
    _sweep(8, tag, 2, dev, monkeypatch, forcing="none")


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_4096_on_white_spectra(tag, dev, monkeypatch):
    """The same sweep at 4096^2, one field: the single-thread fp64 oracle (explicit terms and one step, forward, tangent and
    adjoint) takes about a minute on the host, which is why the size has a test function of its own."""
    try:
        _sweep(4096, tag, 1, dev, monkeypatch)
    finally:
        _release(4096)


# ----------------------------------------------------------------------------- (b) the unmasked kernel forms
@pytest.mark.parametrize("n,tag", [(64, "f64"), (96, "f64"), (80, "f64"), (512, "f64"), (64, "f32"), (512, "f32")])
def test_unmasked_unforced_forms_on_white_spectra(n, tag, dev, monkeypatch):
    """smooth=False, no forcing: unpruned plans with the lone Nyquist tile, no forcing add."""
    _sweep(n, tag, 2, dev, monkeypatch, forcing="none", smooth=False)


# ----------------------------------------------------------------------------- (c) the IMEX schedules
@pytest.mark.parametrize("n,tag", [(64, "f64"), (96, "f32")])
@pytest.mark.parametrize("solver", ["imex1", "imex1.5", "imex2"])
def test_imex_schedules_on_white_spectra(solver, n, tag, dev, monkeypatch):
    """IMEXStepper orders 1, 1.5 and 2, two steps: order 2 restarts its second stage from the step's input."""
    _sweep(n, tag, 2, dev, monkeypatch, solver=solver, steps=2)
