"""4096^2 grids on the fused spectral kernels: every entry point that takes a tcfd_ns2d_plan, both precisions.

Reference: the plain-torch restatement tests/ns2d_ops.py evaluated ON THE DEVICE in fp64 (torch.fft ops on tables built by the
oracle; tests/test_ns2d_jvp_host.py ties it to oracle/ns2d.py and to the goldens) -- the CPU oracle, pinned to one thread, would
take tens of seconds per case at this size; ONE case compares against it all the same, the explicit terms of one fp64 field
(five single-thread 4096^2 transforms: about five seconds).  Inputs: seeded fields built on
the device, a Gaussian spectrum (rms 5) like the fields of the tangent tests, plus a white floor of 1e-6 of the peak amplitude in
every bin: with the Gaussian alone every bin beyond |k| ~ 40 of the 4096 x 2049 half spectrum underflows, and a kernel that
misplaced rows or columns out there would be compared on zeros.

Bounds (rel-L2 unless stated), the project's at 2048^2 (tests/test_ns2d_gpu.py::test_against_oracle) and of
tests/test_ns2d_jvp_gpu.py:
  state, stream function  1e-10 fp64, 4e-6 fp32          explicit terms  1e-10 fp64, 2e-5 fp32
  dw/dt                   1e-8 fp64; fp32 (and fp64 too) the error scaled by |w| / dt, bound of the state
  residual                error scaled by |w_t| + |F| (what cancels in it), bound of the explicit terms
  transforms              1e-13 fp64, 2e-6 fp32
  tangents                1e-10 (explicit terms) / 1e-9 (stepped) fp64, 2e-5 fp32 against the fp64 tangent
  adjoint identity        1e-12 fp64, 1e-5 fp32 relative to |J dw| |g|
  kernel variants         1e-13 state, 1e-12 explicit terms fp64; 5e-7, 2e-6 fp32; a different block -> tile map alone: bitwise
"""
import ctypes
import functools
import math

import pytest
import torch

import ns2d_ops
from guard_ops import Arena, Out, nbytes, run_guarded

pytestmark = pytest.mark.gpu

N, M = 4096, 2049
L = 2 * math.pi
DT = 2.5e-4
REAL = {"f64": torch.float64, "f32": torch.float32}
CPLX = {"f64": torch.complex128, "f32": torch.complex64}
TOL_STATE = {"f64": 1e-10, "f32": 4e-6}
TOL_F = {"f64": 1e-10, "f32": 2e-5}
TCFD_EINVAL = -1


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dev():
    return _dev()


@pytest.fixture(scope="module", autouse=True)
def _release_plans_and_buffers():
    """The operators (tables of 4096 x 2049), inputs and references of this file -- a few GB -- do not outlive it."""
    yield
    for cached in (operator, fields, tables64):
        cached.cache_clear()
    from torch_cfd_amd import equations

    for key in [k for k in equations._MESH_PLANS if k[0] == N]:
        del equations._MESH_PLANS[key]
    torch.cuda.empty_cache()


def nrm(x):
    return torch.linalg.norm(x.reshape(-1).to(torch.complex128 if x.is_complex() else torch.float64)).item()


def rel(a, b):
    """rel-L2 on the device (conftest.rel_l2 copies both arrays to the host: 0.4 GB each at B = 3)."""
    wide = torch.complex128 if b.is_complex() else torch.float64
    return nrm(a.to(wide) - b.to(wide)) / nrm(b)


def make_op(n, tag, forcing, smooth=True, solver=None):
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])
    try:
        grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
        fn = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False) if forcing == "kolmogorov" else None
        solver = {None: tc.RK4CrankNicolsonStepper, "imex2": lambda: tc.IMEXStepper(order=2)}[solver]()
        op = tc.NavierStokes2DSpectral(1e-3, grid, drag=ns2d_ops.DRAG[forcing], smooth=smooth, forcing_fn=fn, solver=solver).to(_dev())
        # the plan samples the forcing when it is built: in the operator's precision, like the tables
        op._plan(torch.zeros(1, dtype=CPLX[tag], device=_dev()))
        return op
    finally:
        torch.set_default_dtype(torch.float32)


@functools.lru_cache(maxsize=None)
def operator(tag, forcing="kolmogorov", smooth=True, solver=None):
    return make_op(N, tag, forcing, smooth, solver)


@functools.lru_cache(maxsize=None)
def tables64(forcing, smooth):
    return ns2d_ops.tables(N, forcing, smooth, device=_dev())


def stepper64(kind=None):
    """The stepper of the reference run: its stage scalars in fp64, whatever the precision of the operator under test."""
    import torch_cfd_amd as tc

    torch.set_default_dtype(torch.float64)
    try:
        return tc.RK4CrankNicolsonStepper() if kind is None else tc.IMEXStepper(order=2)
    finally:
        torch.set_default_dtype(torch.float32)


@functools.lru_cache(maxsize=None)
def fields(n, count, k0, seed):
    """`count` seeded real fields as fp64 half spectra on the device (see the module docstring)."""
    gen = torch.Generator(device=_dev()).manual_seed(seed)
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64, device=_dev())
    env = torch.exp(-(k[:, None] ** 2 + k[None, : n // 2 + 1] ** 2) / (2.0 * k0 * k0)) + 1e-6
    w = torch.fft.irfft2(torch.fft.rfft2(torch.randn(count, n, n, generator=gen, dtype=torch.float64, device=_dev())) * env, s=(n, n))
    return torch.fft.rfft2(5.0 * w / w.std())


def inputs(tag, B):
    """(w0, dw) in the precision of `tag`: up to three distinct samples, repeated with other amplitudes beyond."""
    w0, p0 = fields(N, min(B, 3), 4.0, 1000 + N), fields(N, min(B, 3), 6.0, 2000 + N)
    reps = (B + w0.shape[0] - 1) // w0.shape[0]
    scale = (1 + 0.1 * torch.arange(B, dtype=torch.float64, device=_dev()))[:, None, None]
    return ((w0.repeat(reps, 1, 1)[:B] * scale).to(CPLX[tag]).contiguous(),
            (p0.repeat(reps, 1, 1)[:B] * scale.flip(0)).to(CPLX[tag]).contiguous())


# ----------------------------------------------------------------------------- 1. routing
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_4096_runs_on_the_fused_kernels(tag, dev):
    """The plan of a 4096 grid is a library plan (tcfd_ns2d_plan_create returns 0), not the dense-transform composite."""
    import torch_cfd_amd as tc
    from torch_cfd_amd.equations import _HipPlan, fft_plan

    op = operator(tag)
    plan = op._plan(torch.zeros(1, N, M, dtype=CPLX[tag], device=dev))
    assert isinstance(plan, _HipPlan) and plan.handle.value       # _HipPlan raises unless tcfd_ns2d_plan_create returned 0
    info = plan.info()
    assert "composite" not in info and info["rows_kernel"] == 5 and info["split"] == 1, info
    assert info["keep_cols"] > 0 and info["sparse_forcing"] == 1 and info["separable"] == 1, info
    assert isinstance(fft_plan(N, CPLX[tag], dev), _HipPlan)
    # four fields per chunk (balanced: 5 = 3 + 2); the scratch of a call stops growing at one chunk
    per = ctypes.c_long(0)
    for B, want in ((1, 1), (3, 3), (4, 4), (5, 3), (17, 4), (64, 4)):
        assert plan.lib.tcfd_ns2d_plan_chunking(plan.handle, B, ctypes.byref(per), None, None) == 0 and per.value == want, B
    esz = 16 if tag == "f64" else 8
    ldw = (M + 128 // esz - 1) // (128 // esz) * (128 // esz)
    field = N * ldw * esz                                       # one field in the padded pitch (a multiple of 256 bytes)
    assert field % 256 == 0 and plan.lib.tcfd_ns2d_workspace_bytes(plan.handle, 1) == 8 * field
    assert plan.lib.tcfd_ns2d_workspace_bytes(plan.handle, 8) == 8 * 4 * field == plan.lib.tcfd_ns2d_workspace_bytes(plan.handle, 32)
    assert plan.lib.tcfd_ns2d_workspace_bytes(plan.handle, 64) == 64 * field            # the field of the whole batch irfft2 stages
    assert plan.lib.tcfd_ns2d_jvp_workspace_bytes(plan.handle, 5) == 16 * 2 * field == plan.lib.tcfd_ns2d_jvp_workspace_bytes(plan.handle, 64)
    assert plan.lib.tcfd_irfft2_subsample_max_factor(plan.handle) == 64
    # a batch beyond the 32-bit launch grids is refused before anything is launched; 8192 keeps raising
    x = torch.zeros(16, device=dev)
    limit = (2**31 - 1) // (N + 18)
    assert plan.lib.tcfd_rfft2(plan.handle, x.data_ptr(), x.data_ptr(), limit + 1, None) == TCFD_EINVAL
    assert b"largest batch" in plan.lib.tcfd_last_error()
    assert plan.lib.tcfd_ns2d_velocity(plan.handle, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), limit + 1, None) == TCFD_EINVAL
    with pytest.raises(tc._lib.TcfdError):
        fft_plan(8192, CPLX[tag], dev)


def test_a_library_built_before_the_size_says_rebuild(dev, monkeypatch):
    """The size came without a new ABI number: a stale library loads and answers TCFD_EINVAL at 4096.  The wrapper raises and
    names the remedy instead of routing to something slower."""
    import torch_cfd_amd as tc
    from torch_cfd_amd.equations import _HipPlan

    lib = tc._lib.load()
    monkeypatch.setattr(lib, "tcfd_ns2d_plan_create", lambda *args: TCFD_EINVAL)
    k = torch.fft.fftfreq(N, 1.0 / N, dtype=torch.float64)
    with pytest.raises(tc._lib.TcfdError, match="rebuild"):
        _HipPlan(N, torch.complex64, dev, k, k[:M].abs(), torch.zeros(N, M), torch.ones(N, M))


# ----------------------------------------------------------------------------- 2. transforms
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_transforms_against_torch_fft(tag, dev):
    from torch_cfd_amd.equations import fft_plan

    plan = fft_plan(N, CPLX[tag], dev)
    tol = 1e-13 if tag == "f64" else 2e-6
    gen = torch.Generator(device=dev).manual_seed(41)
    x = torch.randn(2, N, N, generator=gen, dtype=REAL[tag], device=dev)
    xh = plan.rfft2(x)
    ref = torch.fft.rfft2(x.double())
    e_f = rel(xh, ref)
    back = plan.irfft2(xh)
    e_b = rel(back, x)
    # a half spectrum that is NOT the transform of a real field: c2r semantics drop the imaginary parts of the DC and Nyquist
    # columns after the column transform (the reference: the same steps in torch.fft ops, so that its last-axis c2r sees a
    # consistent input whatever the backend does with an inconsistent one)
    z = torch.view_as_complex(torch.randn(2, N, M, 2, generator=gen, dtype=REAL[tag], device=dev))
    y = torch.fft.ifft(z.to(torch.complex128), dim=-2)
    y[..., 0].imag.zero_()
    y[..., M - 1].imag.zero_()
    e_n = rel(plan.irfft2(z), torch.fft.irfft(y, n=N, dim=-1))
    print(f"{tag}: rfft2 {e_f:.3e} irfft2(rfft2 x) {e_b:.3e} irfft2 of a non-Hermitian spectrum {e_n:.3e}")
    assert xh.dtype == CPLX[tag] and back.dtype == REAL[tag]
    assert e_f <= tol and e_b <= tol and e_n <= tol


# ----------------------------------------------------------------------------- 3. explicit terms, RK4-CN step, dw/dt, residual
@pytest.mark.parametrize("forcing,smooth", [("kolmogorov", True), ("none", False)], ids=["kolmogorov-pruned", "unforced-unpruned"])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_step_and_explicit_terms_against_the_fp64_restatement(tag, forcing, smooth, dev):
    """(Kolmogorov forcing, smooth=True): sparse forcing, pruned plan, packed Nyquist column.  (no forcing, smooth=False): the
    unpruned plan with the lone Nyquist tile.  B = 3: one ragged chunk."""
    op = operator(tag, forcing, smooth)
    info = op._plan(torch.zeros(1, N, M, dtype=CPLX[tag], device=dev)).info()
    assert (info["keep_cols"] > 0) == smooth, info
    w0, _ = inputs(tag, 3)
    t = tables64(forcing, smooth)
    w64 = w0.to(torch.complex128)
    F_ref = ns2d_ops.explicit_terms(w64, t)
    ref = ns2d_ops.step(w64, t, ns2d_ops.schedule(stepper64(), DT))
    ref_dt = (ref - w64) / DT
    e_F = rel(op.explicit_terms(w0), F_ref)
    out, dwdt = op(w0, DT, steps=1)
    e_w, e_dt = rel(out, ref), rel(dwdt, ref_dt)
    e_dts = nrm(dwdt.to(torch.complex128) - ref_dt) / (nrm(ref) / DT)
    wt = ref_dt.to(CPLX[tag])
    psi, res = op.stream_and_residual(w0, wt)
    wt64 = wt.to(torch.complex128)
    e_psi = rel(psi, -t.inv_lap * w64)
    res_ref = wt64 - F_ref - t.linear_term * w64
    e_res = nrm(res.to(torch.complex128) - res_ref) / (nrm(wt64) + nrm(F_ref))
    print(f"{tag} {forcing} smooth={smooth}: F {e_F:.3e} w {e_w:.3e} dw/dt {e_dt:.3e} (scaled {e_dts:.3e}) psi {e_psi:.3e} "
          f"residual (scaled) {e_res:.3e}")
    assert e_F <= TOL_F[tag] and e_w <= TOL_STATE[tag]
    if tag == "f64":
        assert e_dt <= 1e-8
    assert e_dts <= TOL_STATE[tag]
    assert e_psi <= TOL_STATE[tag] and e_res <= TOL_F[tag]


def test_explicit_terms_of_one_field_against_the_cpu_oracle(dev):
    """The one CPU comparison at this size: oracle/ns2d.py on one host thread (see tests/test_ns2d_gpu.py::test_against_oracle
    for why one), explicit terms of one fp64 field; bound of that test, 1e-10."""
    from oracle import ns2d as O

    op = operator("f64")
    w0, _ = inputs("f64", 1)
    got = op.explicit_terms(w0).cpu()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    try:
        ref = O.explicit_terms(w0.cpu(), tables64("kolmogorov", True).oracle)
    finally:
        torch.set_num_threads(threads)
        torch.set_default_dtype(torch.float32)
    err = (torch.linalg.norm(got - ref) / torch.linalg.norm(ref)).item()
    print(f"f64 explicit terms against the CPU oracle: {err:.3e}")
    assert err <= 1e-10


# ----------------------------------------------------------------------------- 4. IMEX order 2 (a base0 schedule)
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_imex_order_2_step(tag, dev):
    op = operator(tag, "kolmogorov", True, "imex2")
    ref_stepper = stepper64("imex2")
    sched = ns2d_ops.schedule(ref_stepper, DT)
    assert sched["base0"] is not None and any(sched["base0"])
    w0, _ = inputs(tag, 2)
    w64 = w0.to(torch.complex128)
    ref = ns2d_ops.step(w64, tables64("kolmogorov", True), sched)
    out, dwdt = op(w0, DT, steps=1)
    e_w = rel(out, ref)
    e_dts = nrm(dwdt.to(torch.complex128) - (ref - w64) / DT) / (nrm(ref) / DT)
    print(f"{tag} imex2: w {e_w:.3e} dw/dt (scaled) {e_dts:.3e}")
    assert e_w <= TOL_STATE[tag] and e_dts <= TOL_STATE[tag]


# ----------------------------------------------------------------------------- 5. bitwise
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_steps_chunks_and_reruns_are_bitwise(tag, dev):
    """B = 5: two chunks, of three and of two fields."""
    B = 5
    op = operator(tag)
    w0, _ = inputs(tag, B)
    two, dt2 = op(w0, DT, steps=2)
    again, dt2b = op(w0, DT, steps=2)
    assert torch.equal(two, again) and torch.equal(dt2, dt2b)
    one, _ = op(w0, DT, steps=1)
    assert torch.equal(op(one, DT, steps=1)[0], two)
    F = op.explicit_terms(w0)
    psi, res = op.stream_and_residual(w0, dt2)
    for b in range(B):
        alone, dta = op(w0[b:b + 1], DT, steps=2)
        assert torch.equal(alone[0], two[b]) and torch.equal(dta[0], dt2[b]), b
        assert torch.equal(op.explicit_terms(w0[b:b + 1])[0], F[b]), b
        pa, ra = op.stream_and_residual(w0[b:b + 1], dt2[b:b + 1])
        assert torch.equal(pa[0], psi[b]) and torch.equal(ra[0], res[b]), b


def test_a_sample_past_two_gib_of_the_batch_is_bitwise_its_run_alone(dev):
    """fp64, B = 17 (chunks of 4, 4, 4, 4 and 1): sample 16 starts 2^31 + 1.1e6 bytes into the arrays (134 283 264 bytes per field)."""
    op = operator("f64")
    w0, _ = inputs("f64", 17)
    assert 16 * N * M * 16 > 2**31
    F = op.explicit_terms(w0)
    for b in (16, 15):
        assert torch.equal(op.explicit_terms(w0[b:b + 1])[0], F[b]), b
    assert bool(torch.isfinite(torch.view_as_real(F)).all())


# ----------------------------------------------------------------------------- 6. forward and reverse mode
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_tangents_against_forward_mode_of_the_restatement(tag, dev):
    op = operator(tag)
    w0, dw = inputs(tag, 2)
    t = tables64("kolmogorov", True)
    w64, d64 = w0.to(torch.complex128), dw.to(torch.complex128)
    F_ref, dF_ref = ns2d_ops.jvp(lambda w: ns2d_ops.explicit_terms(w, t), w64, d64)
    sched = ns2d_ops.schedule(stepper64(), DT)
    w_ref, dw_ref = ns2d_ops.jvp(lambda w: ns2d_ops.step(w, t, sched), w64, d64)
    f, df = op.explicit_terms_jvp(w0, dw)
    w1, d1 = op.tangent_step(w0, dw, DT, 1)
    errs = {"F": rel(f, F_ref), "dF": rel(df, dF_ref), "w": rel(w1, w_ref), "dw": rel(d1, dw_ref)}
    e_p = rel(w1, op(w0, DT, steps=1)[0])
    print(f"{tag}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" primal-vs-step {e_p:.3e}")
    tol_f, tol_s, tol_p = (1e-10, 1e-9, 1e-12) if tag == "f64" else (2e-5, 2e-5, 2e-5)
    assert errs["F"] <= tol_f and errs["dF"] <= tol_f and errs["w"] <= tol_s and errs["dw"] <= tol_s and e_p <= tol_p
    # zero tangent -> zero tangent, and the primal does not see the tangent
    fz, dfz = op.explicit_terms_jvp(w0, torch.zeros_like(dw))
    wz, dz = op.tangent_step(w0, torch.zeros_like(dw), DT, 1)
    assert bool((dfz == 0).all()) and bool((dz == 0).all()) and torch.equal(fz, f) and torch.equal(wz, w1)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_adjoint_identity_between_the_fused_jvp_and_vjp(tag, dev):
    """<J dw, g> = <dw, J^T g>: J dw from the tangent kernels, J^T g from the reverse-mode kernels
    (tcfd_ns2d_explicit_terms_vjp, tcfd_ns2d_stage_update_vjp), explicit terms and one step."""
    op = operator(tag)
    w0, dw = inputs(tag, 1)
    gen = torch.Generator(device=dev).manual_seed(N)
    g = torch.view_as_complex(torch.randn(1, N, M, 2, generator=gen, dtype=torch.float64, device=dev)).to(CPLX[tag])
    tol = 1e-12 if tag == "f64" else 1e-5
    for what, jdw, forward in (("explicit", op.explicit_terms_jvp(w0, dw)[1], op.explicit_terms),
                               ("step", op.tangent_step(w0, dw, DT, 1)[1], lambda w: op(w, DT, 1)[0])):
        w = w0.clone().requires_grad_(True)
        jtg, = torch.autograd.grad(ns2d_ops.real_inner(g, forward(w)), w)
        lhs, rhs = ns2d_ops.real_inner(jdw, g).item(), ns2d_ops.real_inner(dw, jtg).item()
        scale = nrm(jdw) * nrm(g)
        print(f"{tag} {what}: <Jdw,g> {lhs:.12e} <dw,JTg> {rhs:.12e} defect/scale {abs(lhs - rhs) / scale:.3e}")
        assert abs(lhs - rhs) <= tol * scale, what


# ----------------------------------------------------------------------------- 7. irfft2 + bilinear subsample, 4096 -> 512
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_fused_subsample_4096_to_512(tag, dev):
    """Held to what tests/test_ns2d_gpu.py::test_fused_c2r_subsample_is_bit_identical_to_the_two_steps asserts for a factor
    beyond 2: rounding against the library's own two steps, 2e-6 / 1e-14 against torch.fft + F.interpolate."""
    from torch_cfd_amd.data_gen import spectral_to_physical
    from torch_cfd_amd.equations import fft_plan

    plan = fft_plan(N, CPLX[tag], dev)
    top = plan.lib.tcfd_irfft2_subsample_max_factor(plan.handle)
    assert top == 64 and plan.subsample_factor(512) == 8 and plan.subsample_factor(N // top) == top
    assert plan.subsample_factor(N // (2 * top)) == 0 and plan.subsample_factor(N) == 0
    gen = torch.Generator(device=dev).manual_seed(512)
    x = torch.randn(2, N, N, generator=gen, dtype=REAL[tag], device=dev)
    xh = torch.fft.rfft2(x)
    fused = plan.irfft2_subsample(xh, 8)
    interp = lambda v: torch.nn.functional.interpolate(v.reshape(-1, 1, N, N), size=(512, 512), mode="bilinear").reshape(2, 512, 512)
    e_two, e_ref = rel(fused, interp(plan.irfft2(xh))), rel(fused, interp(torch.fft.irfft2(xh, s=(N, N))))
    print(f"{tag}: against the two library calls {e_two:.3e}, against torch.fft + interpolate {e_ref:.3e}")
    assert fused.shape == (2, 512, 512) and fused.dtype == REAL[tag]
    assert e_two < (3e-7 if tag == "f32" else 5e-16) and e_ref < (2e-6 if tag == "f32" else 1e-14)
    assert torch.equal(spectral_to_physical(xh, 512, REAL[tag]), fused)


# ----------------------------------------------------------------------------- 8. variants
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_split_and_whole_column_tiles_agree_at_4096(tag, dev, monkeypatch):
    """TCFD_SPLIT=0: the step's column passes on whole-column tiles (one fp64 / two fp32 columns, line groups of eight) instead
    of the 2048-point halves: the same arithmetic in another order."""
    w0, _ = inputs(tag, 2)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("TCFD_SPLIT", flag)      # read at plan creation: a new operator is a new plan
        op = make_op(N, tag, "kolmogorov")
        assert op._plan(w0).info()["split"] == int(flag)
        res[flag] = (op(w0, DT, steps=1)[0], op.explicit_terms(w0))
        del op
    monkeypatch.delenv("TCFD_SPLIT")
    default = operator(tag)
    assert torch.equal(default(w0, DT, steps=1)[0], res["1"][0])
    e_w, e_F = rel(res["0"][0], res["1"][0]), rel(res["0"][1], res["1"][1])
    print(f"{tag}: whole-column against split: w {e_w:.3e} F {e_F:.3e}")
    tol_w, tol_F = (1e-13, 1e-12) if tag == "f64" else (5e-7, 2e-6)
    assert e_w < tol_w and e_F < tol_F


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_line_groups_of_eight_at_256(tag, dev, monkeypatch):
    """TCFD_PAIR_XCD=8 (the block -> tile map of the 16-byte tiles of n = 4096, forced on the narrow tiles of a small grid)
    against the default groups of 2 / 4 and against no grouping: the same tiles in another launch order -- every bit equal.
    n = 256, B = 4 runs the 4-column tiles (32 / 64 bytes); B = 5 leaves the last group of eight short."""
    n = 256
    for B in (4, 5):
        w0 = fields(n, 3, 4.0, 77).repeat(2, 1, 1)[:B].to(CPLX[tag]).contiguous()
        res = {}
        for flag in ("8", "1", "0"):
            monkeypatch.setenv("TCFD_PAIR_XCD", flag)
            op = make_op(n, tag, "kolmogorov")
            out, dwdt = op(w0, 1e-3, steps=2)
            f, df = op.explicit_terms_jvp(w0, w0.flip(0))
            res[flag] = (out, dwdt, op.explicit_terms(w0), f, df)
        monkeypatch.delenv("TCFD_PAIR_XCD")
        for flag in ("1", "0"):
            for a, b in zip(res["8"], res[flag]):
                assert torch.equal(a, b), (B, flag)
        ref = ns2d_ops.advance(w0.to(torch.complex128), ns2d_ops.tables(n, "kolmogorov", True, device=dev),
                               ns2d_ops.schedule(stepper64(), 1e-3), steps=2)
        assert rel(res["8"][0], ref) <= TOL_STATE[tag]


# ----------------------------------------------------------------------------- 9. memory contract
def _guard(what, ins, outs, call, need, baseline):
    """One guarded call (tests/guard_ops.py): exactly `need` bytes of scratch between moats, poisoned three ways."""
    regions = [(k, nbytes(t.dtype, t.shape)) for k, t in ins.items()] + [("ws", int(need))]
    regions += [(k, nbytes(o.dtype, o.shape)) for k, o in outs.items() if k not in ins]
    arena = Arena(_dev(), regions)
    from torch_cfd_amd import _lib

    def run(ws_bytes):
        with torch.cuda.device(_dev()):
            return call(lambda name: arena.ptr(name) if name is not None else None, arena.ptr("ws"), ws_bytes)

    return run_guarded(run, arena, ins, outs, "ws", need=int(need), baseline=baseline, last_error=_lib.load().tcfd_last_error,
                       what=what)


@pytest.mark.parametrize("what", ["step", "explicit_terms_jvp", "irfft2"])
def test_memory_contract_at_4096(what, dev):
    """4096^2 x 2 fp32 inside a guarded arena, with exactly the scratch the size functions report: the moats and the poison
    outside the reported extents stay intact, the outputs are written in full and do not depend on what the scratch held."""
    from torch_cfd_amd import _lib

    op = operator("f32")
    w, dw = inputs("f32", 2)
    plan, lib = op._plan(w), _lib.load()
    h, B = plan.handle, 2
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cplx = Out(torch.complex64, (B, N, M))
    if what == "step":
        sc = op._schedule(op.solver, op.solver.params, DT)
        beta, gdt, mu = (_lib.darray(sc[k]) for k in ("beta", "gdt", "mu"))
        ref = plan.step(w, sc["beta"], sc["gdt"], sc["mu"], 1, 1 / DT, True)
        _guard("tcfd_ns2d_step", {"w": w}, {"out": cplx, "dwdt": cplx},
               lambda P, ws, nb: lib.tcfd_ns2d_step(h, P("w"), P("out"), P("dwdt"), B, len(sc["beta"]), beta, gdt, mu, 1, 1 / DT, ws,
                                                    nb, stream),
               lib.tcfd_ns2d_workspace_bytes(h, B), {"out": ref[0], "dwdt": ref[1]})
    elif what == "explicit_terms_jvp":
        f, df = plan.explicit_terms_jvp(w, dw)
        _guard("tcfd_ns2d_explicit_terms_jvp", {"w": w, "dw": dw}, {"f": cplx, "df": cplx},
               lambda P, ws, nb: lib.tcfd_ns2d_explicit_terms_jvp(h, P("w"), P("dw"), P("f"), P("df"), B, ws, nb, stream),
               lib.tcfd_ns2d_jvp_workspace_bytes(h, B), {"f": f, "df": df})
    else:
        # the prefix rule of include/tcfd.h: one field of the whole batch in the padded pitch
        need = (B * N * 2064 * 8 + 255) // 256 * 256
        assert need <= lib.tcfd_ns2d_workspace_bytes(h, B)
        _guard("tcfd_irfft2", {"w": w}, {"out": Out(torch.float32, (B, N, N))},
               lambda P, ws, nb: lib.tcfd_irfft2(h, P("w"), P("out"), B, ws, nb, stream), need, {"out": plan.irfft2(w)})
