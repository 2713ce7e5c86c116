"""GPU tests of ensembles with per-sample viscosity, drag and forcing amplitude (``tcfd_ns2d_plan_set_ensemble``): member b of one
ensemble call against (1) the reference's scalar runs (tests/golden/ns2d_ensemble.npz), per member, (2) a scalar operator of
the same build on every kernel form, (3) the batch plumbing -- chunks, graph replay, half-batch overlap, (B, T, n, m) --, the
IMEX orders, reverse mode, the loud refusals, the untouched scalar path and the data generator.

Tolerances (rel-L2 per member) are those of ``test_ns2d_gpu.py::test_golden_steps`` for the scalar path: fp64 1e-10; fp32 2e-6
for F and one step, 1e-5 for ten steps; dw/dt and the residual in that test's ``scaled_err`` forms at the same bounds.
"""
import math

import pytest
import torch

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

L = 2 * math.pi
DT = 1e-3
REAL = {"f64": torch.float64, "f32": torch.float32}
CPLX = {"f64": torch.complex128, "f32": torch.complex64}
NU = (1e-3, 1e-2, 5e-2, 2e-1)
DRAG = (0.1, 0.0, 0.5, 0.05)
FSCALE = (1.0, 0.0, -2.0, 0.5)
ONES = (1.0, 1.0, 1.0, 1.0)
B = 4
T1 = {"f64": 1e-10, "f32": 2e-6}     # F, one step
T10 = {"f64": 1e-10, "f32": 1e-5}    # ten steps


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return load_golden("ns2d_ensemble.npz")


def scaled_err(a, b, scale_of):
    """||a - b|| / ||scale_of|| (test_ns2d_gpu.py): the error of a difference of larger terms against the terms that cancel."""
    a, b, s = (torch.as_tensor(x).to("cpu", torch.complex128) for x in (a, b, scale_of))
    return (torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(s.reshape(-1))).item()


def wave_number(n):
    """4, the wave number of the goldens, wherever the grid resolves it; 2 at n = 8, where 4 is the Nyquist mode: sin(4 y) samples
    to round-off in every bin there, which a forcing scale of 0 turns into exact zeros -- another plan (pruned, sparse forcing)
    than the members with a non-zero scale get, and nothing of a forcing to compare."""
    return 4 if n >= 16 else 2


def ensemble_op(n, tag, dev, nu=NU, drag=DRAG, fscale=FSCALE, solver=None):
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=wave_number(n), swap_xy=False)
    return tc.NavierStokes2DSpectral(list(nu), grid, drag=list(drag), smooth=True, forcing_fn=forcing, forcing_scale=list(fscale),
                                     solver=solver or tc.RK4CrankNicolsonStepper()).to(dev)


def scalar_op(n, tag, dev, nu, drag, fscale, solver=None):
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=fscale, wave_number=wave_number(n), swap_xy=False)
    return tc.NavierStokes2DSpectral(nu, grid, drag=drag, smooth=True, forcing_fn=forcing,
                                     solver=solver or tc.RK4CrankNicolsonStepper()).to(dev)


def random_state(n, count, tag, dev, seed=7):
    """Half spectra of `count` real white-noise fields: every mode is live, the Nyquist row and column included."""
    gen = torch.Generator().manual_seed(seed + n)
    x = torch.randn(count, n, n, generator=gen, dtype=torch.float64)
    return torch.fft.rfft2(x).to(CPLX[tag]).to(dev)


def per_member(fn, out, ref, tol, what):
    errs = [fn(out[b], ref[b]) for b in range(out.shape[0])]
    print(what, " ".join(f"{e:.2e}" for e in errs))
    for b, e in enumerate(errs):
        assert e < tol, (what, b, e, tol)


# ----------------------------------------------------------------------------- 1. golden parity, per member
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_golden_parity_per_member(tag, dev, golden):
    g = golden
    w0c = torch.from_numpy(g["f64_w0"]).to(CPLX[tag])
    ref = {k: torch.from_numpy(g[f"{tag}_{k}"]) for k in ("F", "w1", "w10", "res1")}
    # the reference forms dw/dt as 1 / (steps dt) * (w_new - w0): the generator asserts the stored states give it bit for bit
    d1_ref, d10_ref = 1 / (1 * DT) * (ref["w1"] - w0c), 1 / (10 * DT) * (ref["w10"] - w0c)
    op = ensemble_op(64, tag, dev)
    w0 = w0c.to(dev)
    t1, t10 = T1[tag], T10[tag]
    F = op.explicit_terms(w0)
    assert F.dtype == CPLX[tag] and F.shape == w0.shape
    per_member(rel_l2, F.cpu(), ref["F"], t1, "F")
    w1, d1 = op(w0, DT)
    per_member(rel_l2, w1.cpu(), ref["w1"], t1, "w1")
    for b in range(B):
        assert scaled_err(d1[b], d1_ref[b], ref["w1"][b] / 1e-3) < t1, b
    w10, d10 = op(w0, DT, steps=10)
    per_member(rel_l2, w10.cpu(), ref["w10"], t10, "w10")
    for b in range(B):
        assert scaled_err(d10[b], d10_ref[b], ref["w1"][b] / 1e-2) < t10, b
    res1 = op.residual(w1, d1)
    for b in range(B):
        assert scaled_err(res1[b], ref["res1"][b], d1_ref[b]) < (1e-10 if tag == "f64" else 3e-4), b
    # ten single-step calls equal steps=10
    w = w0
    for _ in range(10):
        w, _ = op(w, DT)
    per_member(rel_l2, w.cpu(), w10.cpu(), 1e-14 if tag == "f64" else 1e-6, "10 x 1 vs steps=10")
    # the reference's broadcasting form of the constructor is the same operator
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(64, 64), domain=((0, L), (0, L)))
    op2 = tc.NavierStokes2DSpectral(torch.tensor(NU).view(B, 1, 1), grid, drag=torch.tensor(DRAG).view(B, 1, 1), smooth=True,
                                    forcing_fn=tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4, swap_xy=False),
                                    forcing_scale=torch.tensor(FSCALE), solver=tc.RK4CrankNicolsonStepper()).to(dev)
    assert torch.equal(op2(w0, DT)[0], w1)
    assert op.linear_term.shape == (B, 64, 33)
    assert torch.equal(op.linear_term, op.viscosity * op.laplace - op.drag)


# ----------------------------------------------------------------------------- 2. same build, every kernel form
def _compare_with_scalar_ops(n, tag, dev, fscale, bit_equal):
    w0 = random_state(n, B, tag, dev)
    op = ensemble_op(n, tag, dev, fscale=fscale)
    out, dwdt = op(w0, DT, steps=3)
    F = op.explicit_terms(w0)
    res = op.residual(out, dwdt)
    info = op._plan(w0).info()
    for b in range(B):
        sop = scalar_op(n, tag, dev, NU[b], DRAG[b], fscale[b])
        so, sd = sop(w0[b:b + 1], DT, steps=3)
        sF = sop.explicit_terms(w0[b:b + 1])
        sres = sop.residual(so, sd)
        assert sop._plan(w0[b:b + 1]).info() == info     # the same kernels on both sides
        if bit_equal:
            assert torch.equal(out[b:b + 1], so), (n, tag, b, rel_l2(out[b:b + 1], so))
            assert torch.equal(dwdt[b:b + 1], sd), (n, tag, b)
            assert torch.equal(F[b:b + 1], sF), (n, tag, b)
            assert torch.equal(res[b:b + 1], sres), (n, tag, b)
        else:
            assert rel_l2(out[b:b + 1], so) < T1[tag], (n, tag, b)
            assert rel_l2(F[b:b + 1], sF) < T1[tag], (n, tag, b)
            assert scaled_err(dwdt[b:b + 1], sd, so / 3e-3) < T1[tag], (n, tag, b)
            assert scaled_err(res[b:b + 1], sres, sd) < (1e-10 if tag == "f64" else 3e-4), (n, tag, b)
    return info


@pytest.mark.parametrize("n", [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 96, 192, 384, 768, 1536, 80, 160, 320, 640, 1280])
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("scales", ["ones", "scaled"])
def test_member_equals_scalar_operator(n, tag, scales, dev):
    """Member b of one ensemble call against a scalar operator (nu_b, drag_b) of the same build on a batch of one, 3 steps, on a
    white state (``random_state``), at every fused size up to 2048: the scalar kernels of each size are held to the CPU oracle on
    full-band spectra by tests/test_ns2d_white_spectrum_gpu.py.  With forcing scales of 1 both sides evaluate the same roundings:
    the same bits.

    n = 8 steps its member of forcing scale 0 with scale 0.25 instead: a plan keeps its forcing as a sparse list while
    ``64 nnz <= n m``, which on the 40 bins of that grid only the empty list of a zero forcing meets, so the scalar twin of a
    zero-scale member runs the sparse form next to the ensemble's dense table and "the same kernels on both sides" cannot hold.
    Every other size keeps the zero member."""
    fscale = ONES if scales == "ones" else FSCALE
    if n == 8:
        fscale = tuple(f or 0.25 for f in fscale)
    _compare_with_scalar_ops(n, tag, dev, fscale, bit_equal=scales == "ones")


@pytest.mark.parametrize("var,value,n", [("TCFD_FORCE_TABLES", "1", 128), ("TCFD_NO_PRUNE", "1", 128), ("TCFD_NYQ_PACK", "0", 128),
                                         ("TCFD_SPLIT", "0", 1024)])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_member_equals_scalar_operator_on_the_other_kernel_forms(var, value, n, tag, dev, monkeypatch):
    monkeypatch.setenv(var, value)     # read at plan creation: every operator below builds its plan under it
    info = _compare_with_scalar_ops(n, tag, dev, ONES, bit_equal=True)
    _compare_with_scalar_ops(n, tag, dev, FSCALE, bit_equal=False)
    if var == "TCFD_FORCE_TABLES":
        assert info["separable"] == 0 and info["sparse_forcing"] == 0     # dense linear term, dense forcing
    if var == "TCFD_NO_PRUNE":
        assert info["keep_cols"] == 0
    if var == "TCFD_SPLIT":
        assert info["split"] == 0


# ----------------------------------------------------------------------------- 3. batch plumbing, bit-identical
NU6 = (1e-3, 1e-2, 5e-2, 2e-1, 3e-3, 7e-2)
DRAG6 = (0.1, 0.0, 0.5, 0.05, 0.2, 0.3)
FS6 = (1.0, 0.0, -2.0, 0.5, 1.5, -1.0)


@pytest.fixture(scope="module")
def plumbing_reference(dev):
    """The default run every plumbing variant must reproduce bit for bit (n = 64, B = 6, fp64), computed once."""
    w0 = random_state(64, 6, "f64", dev, seed=11)
    op = ensemble_op(64, "f64", dev, NU6, DRAG6, FS6)
    out, dwdt = op(w0, DT, steps=5)
    F = op.explicit_terms(w0)
    res = op.residual(out, dwdt)
    torch.cuda.synchronize()
    return w0, out.clone(), dwdt.clone(), F.clone(), res.clone()


@pytest.mark.parametrize("var,value", [("TCFD_CHUNK", "1"), ("TCFD_CHUNK", "4"), ("TCFD_OVERLAP", "1")])
def test_chunks_and_overlap_use_the_callers_batch_index(var, value, dev, monkeypatch, plumbing_reference):
    w0, out, dwdt, F, res = plumbing_reference
    monkeypatch.setenv(var, value)
    op = ensemble_op(64, "f64", dev, NU6, DRAG6, FS6)
    o, d = op(w0, DT, steps=5)
    assert torch.equal(o, out) and torch.equal(d, dwdt)
    assert torch.equal(op.explicit_terms(w0), F)
    assert torch.equal(op.residual(o, d), res)
    if var == "TCFD_CHUNK":
        import ctypes

        plan, per = op._plan(w0), ctypes.c_long(0)
        assert plan.lib.tcfd_ns2d_plan_chunking(plan.handle, 6, ctypes.byref(per), None, None) == 0
        assert per.value == {"1": 1, "4": 3}[value]      # 4 fields per chunk: two balanced chunks of 3


def test_graph_replay_and_a_changed_viscosity(dev, monkeypatch, plumbing_reference):
    w0, out, dwdt, _, _ = plumbing_reference
    monkeypatch.setenv("TCFD_GRAPH", "1")
    op = ensemble_op(64, "f64", dev, NU6, DRAG6, FS6)
    o, d = op(w0, DT, steps=5)
    assert torch.equal(o, out) and torch.equal(d, dwdt)
    o2, _ = op(w0, DT, steps=5)       # same key: replayed
    assert torch.equal(o2, out)
    new_nu = tuple(reversed(NU6))
    with torch.no_grad():
        op.viscosity.copy_(torch.tensor(new_nu, device=dev).view(6, 1, 1))
    o3, d3 = op(w0, DT, steps=5)      # the captured graph must not outlive the table
    monkeypatch.delenv("TCFD_GRAPH")
    fresh = ensemble_op(64, "f64", dev, new_nu, DRAG6, FS6)
    f3, fd3 = fresh(w0, DT, steps=5)
    assert torch.equal(o3, f3) and torch.equal(d3, fd3)
    assert not torch.equal(o3, out)


def test_time_slices_use_their_samples_member(dev):
    """(B, T, n, m): every time slice of sample b steps with member b -- the flattened call with every value repeated T times."""
    T = 3
    w = random_state(64, 6 * T, "f64", dev, seed=13).reshape(6, T, 64, 33)
    op = ensemble_op(64, "f64", dev, NU6, DRAG6, FS6)
    out, dwdt = op(w, DT, steps=2)
    assert out.shape == w.shape

    def rep(v):
        return [x for x in v for _ in range(T)]

    flat = ensemble_op(64, "f64", dev, rep(NU6), rep(DRAG6), rep(FS6))
    fo, fd = flat(w.reshape(6 * T, 64, 33), DT, steps=2)
    assert torch.equal(out.reshape(fo.shape), fo) and torch.equal(dwdt.reshape(fd.shape), fd)
    assert torch.equal(op.explicit_terms(w).reshape(fo.shape), flat.explicit_terms(w.reshape(6 * T, 64, 33)))
    assert torch.equal(op.implicit_terms(w), (op.linear_term.unsqueeze(1) * w))
    # and back to (B, n, m) on the same operator
    o1, _ = op(w[:, 0].contiguous(), DT, steps=2)
    assert torch.equal(o1, out[:, 0])


# ----------------------------------------------------------------------------- 4. IMEX orders
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("order", [1, 1.5, 2])
def test_imex_orders(order, tag, dev, golden):
    import torch_cfd_amd as tc

    torch.set_default_dtype(REAL[tag])     # the stepper's coefficient tensors take the default dtype at construction
    w0 = torch.from_numpy(golden["f64_w0"]).to(CPLX[tag]).to(dev)
    alpha = 1.0 if order == 1 else 0.5
    op = ensemble_op(64, tag, dev, solver=tc.IMEXStepper(order=order, alpha=alpha))
    out, dwdt = op(w0, DT)
    if order == 2:
        per_member(rel_l2, out.cpu(), torch.from_numpy(golden[f"{tag}_imex2"]), T1[tag], "imex2")
    for b in range(B):
        sop = scalar_op(64, tag, dev, NU[b], DRAG[b], FSCALE[b], solver=tc.IMEXStepper(order=order, alpha=alpha))
        so, sd = sop(w0[b:b + 1], DT)
        assert rel_l2(out[b:b + 1], so) < T1[tag], (order, b)
        assert scaled_err(dwdt[b:b + 1], sd, so / 1e-3) < T1[tag], (order, b)
    # the generic (tensor-op) form of the step broadcasts the per-sample linear term
    gen = op.solver.stepper(w0, DT, op)
    per_member(rel_l2, gen, out, 1e-12 if tag == "f64" else 2e-6, "generic stepper")


# ----------------------------------------------------------------------------- 5. reverse mode
def _node_names(fn):
    seen, stack, names = set(), [fn], []
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        stack.extend(g for g, _ in f.next_functions)
    return names


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_gradient_with_respect_to_the_state(tag, dev, golden):
    w0 = torch.from_numpy(golden["g32_w0"]).to(CPLX[tag]).to(dev).requires_grad_(True)
    op = ensemble_op(32, tag, dev)
    w3, _ = op(w0, DT, steps=3)
    names = _node_names(w3.grad_fn)
    assert not any("FusedSteps" in s or "StageUpdate" in s or "FusedExplicitTerms" in s for s in names), sorted(set(names))
    (w3.abs() ** 2).sum().backward()
    per_member(rel_l2, w0.grad.cpu(), torch.from_numpy(golden[f"{tag}_g32_grad"]), 1e-9 if tag == "f64" else 2e-5, "grad")
    # the differentiable step is the fused step
    with torch.no_grad():
        plain, _ = op(w0.detach(), DT, steps=3)
    per_member(rel_l2, w3.detach(), plain, 1e-12 if tag == "f64" else 2e-6, "autograd forward vs fused")


# ----------------------------------------------------------------------------- 6. loud errors
def test_loud_errors(dev):
    import torch.autograd.forward_ad as fwAD

    import torch_cfd_amd as tc

    op = ensemble_op(64, "f64", dev)
    w = random_state(64, B, "f64", dev)
    with pytest.raises(ValueError, match=r"B = 4.*\(3,\)"):
        op(w[:3], DT)
    with pytest.raises(ValueError, match=r"B = 4.*\(\)"):
        op(w[0], DT)                    # an unbatched state
    with pytest.raises(ValueError, match="B = 4"):
        op.explicit_terms(w[:2])
    with pytest.raises(ValueError, match="B = 4"):
        op.residual(w[:2], w[:2])
    with pytest.raises(ValueError, match="B = 4"):
        op.implicit_solve(w[:2], 0.1)
    for call in (lambda: op.tangent_step(w, w, DT), lambda: op.explicit_terms_jvp(w, w), lambda: op.adjoint_step(w, w, DT)):
        with pytest.raises(NotImplementedError, match="per-sample parameters"):
            call()
    with fwAD.dual_level():
        dual = fwAD.make_dual(w, w.clone())
        for call in (lambda: op(dual, DT), lambda: op.explicit_terms(dual), lambda: op.residual(dual, dual)):
            with pytest.raises(NotImplementedError, match="per-sample parameters"):
                call()
    grid = tc.Grid(shape=(64, 64), domain=((0, L), (0, L)))
    for kw in ({"viscosity": torch.tensor(NU, requires_grad=True)}, {"viscosity": list(NU), "drag": torch.tensor(DRAG, requires_grad=True)},
               {"viscosity": list(NU), "forcing_scale": torch.tensor(FSCALE, requires_grad=True)}):
        with pytest.raises(NotImplementedError, match="requires grad"):
            tc.NavierStokes2DSpectral(grid=grid, solver=tc.RK4CrankNicolsonStepper(), **kw)
    op.viscosity.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="requires grad"):
        op(w, DT)
    op.viscosity.requires_grad_(False)
    # a composite grid size names its limit
    grid48 = tc.Grid(shape=(48, 48), domain=((0, L), (0, L)))
    op48 = tc.NavierStokes2DSpectral(list(NU), grid48, solver=tc.RK4CrankNicolsonStepper()).to(dev)
    with pytest.raises(NotImplementedError, match="fused grid sizes"):
        op48(random_state(48, B, "f64", dev), DT)
    # the C ABI: batch != count names both numbers, the tangent-linear step names the limit
    plan = op._plan(w)
    with pytest.raises(tc._lib.TcfdError, match=r"batch 3 .* 4 fields"):
        plan.explicit_terms(w[:3].contiguous())
    with pytest.raises(tc._lib.TcfdError, match=r"batch 2 .* 4 fields"):
        plan.step(w[:2].contiguous(), [0.0], [DT], [DT / 2], 1, 1 / DT)
    with pytest.raises(tc._lib.TcfdError, match=r"batch 5 .* 4 fields"):
        w5 = random_state(64, 5, "f64", dev)
        plan.stream_residual(w5, w5)
    with pytest.raises(tc._lib.TcfdError, match="step_jvp.*per-sample parameters"):
        plan.step_jvp(w, w.clone(), [0.0], [DT], [DT / 2], 1)
    with pytest.raises(tc._lib.TcfdError, match="per-sample parameters"):
        plan.explicit_terms_vjp(w, w.clone())
    assert plan.lib.tcfd_ns2d_plan_set_ensemble(plan.handle, -1, None, None, None, None) == -1     # TCFD_EINVAL
    assert plan.lib.tcfd_ns2d_plan_set_ensemble(plan.handle, 2, None, None, None, None) == -1
    out, _ = op(w, DT)                   # the refused calls left the plan as it was
    assert torch.isfinite(torch.view_as_real(out)).all()


# ----------------------------------------------------------------------------- 7. the scalar path is untouched
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_scalar_plan_keeps_its_bits_around_set_ensemble(tag, dev):
    n = 128
    sop = scalar_op(n, tag, dev, 1e-3, 0.1, 1.0)
    w0 = random_state(n, B, tag, dev)
    before, dbefore = sop(w0, DT, steps=3)
    F = sop.explicit_terms(w0)
    plan = sop._plan(w0)
    plan.set_ensemble(sop.laplace, list(NU), list(DRAG), list(FSCALE))
    during, _ = sop(w0, DT, steps=3)
    assert not torch.equal(during, before)                   # the mode is on: other physics
    assert torch.equal(during, ensemble_op(n, tag, dev)(w0, DT, steps=3)[0])
    plan.set_ensemble(None, [], [], [])                      # count = 0: a scalar plan again
    after, dafter = sop(w0, DT, steps=3)
    assert torch.equal(after, before) and torch.equal(dafter, dbefore)
    assert torch.equal(sop.explicit_terms(w0), F)
    a2, _ = sop(w0[:2], DT, steps=3)                         # and any batch again
    assert torch.equal(a2, before[:2])


# ----------------------------------------------------------------------------- 8. the data generator
def test_kolmogorov_dataset_with_a_viscosity_sequence(dev):
    import torch_cfd_amd as tc
    from torch_cfd_amd import data_gen
    from torch_cfd_amd.distributed import TRAJECTORY_FIELDS

    torch.set_default_dtype(torch.float64)
    nus = [1e-3, 1e-2, 5e-2, 2e-1]
    kw = dict(n=64, total_samples=4, batch_size=2, dt=DT, warmup_steps=2, total_steps=4, record_every_steps=2,
              dtype=torch.float64, cdtype=torch.complex128, device=dev)
    data = data_gen.generate_kolmogorov_dataset(viscosity=nus, **kw)
    assert torch.equal(data["viscosity"], torch.tensor(nus, dtype=torch.float64))
    assert "drag" not in data and "scale" not in data
    for j, nu in enumerate(nus):
        one = data_gen.generate_kolmogorov_dataset(viscosity=nu, **kw)
        assert set(one) == set(TRAJECTORY_FIELDS) | {"random_states"}          # a scalar call: exactly today's keys
        assert set(data) == set(one) | {"viscosity"}
        assert rel_l2(data["vorticity"][j], one["vorticity"][j]) < 1e-10, j
        assert rel_l2(data["stream"][j], one["stream"][j]) < 1e-10, j
        assert scaled_err(data["vort_t"][j], one["vort_t"][j], one["vorticity"][j] / 1e-3) < 1e-10, j
    # drag and scale sequences ride along
    both = data_gen.generate_kolmogorov_dataset(viscosity=1e-3, drag=[0.1, 0.2, 0.3, 0.4], scale=[1.0, 2.0, 0.5, -1.0], **kw)
    assert set(both) == set(TRAJECTORY_FIELDS) | {"random_states", "drag", "scale"}
    one = data_gen.generate_kolmogorov_dataset(viscosity=1e-3, drag=0.3, scale=0.5, **kw)
    assert rel_l2(both["vorticity"][2], one["vorticity"][2]) < 1e-10
    with pytest.raises(ValueError, match="total_samples = 4"):
        data_gen.generate_kolmogorov_dataset(viscosity=[1e-3, 1e-2], **kw)


# ----------------------------------------------------------------------------- the C ABI on its own, and the example
def test_c_abi_ensemble_without_python(dev, tmp_path):
    """examples/c_abi_ensemble_taylor_green.c: plain C99 + HIP runtime, no Python in the process.  Three members with their own
    (nu, drag) decay at their own analytic Taylor-Green rates in one tcfd_ns2d_step call; the program also checks the batch !=
    count refusal and that count = 0 gives back the scalar plan."""
    import os
    import shutil
    import subprocess

    from conftest import ROOT

    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc / ROCm headers")
    import torch_cfd_amd as tc

    tc._lib.load()
    csrc = os.path.join(ROOT, "torch-cfd_amd", "csrc")
    exe = str(tmp_path / "c_abi_ensemble_taylor_green")
    cmd = [gcc, "-std=c99", "-O2", os.path.join(ROOT, "examples", "c_abi_ensemble_taylor_green.c"), "-I" + os.path.join(ROOT, "include"),
           "-I/opt/rocm/include", "-L" + csrc, "-L/opt/rocm/lib", "-ltcfd_hip", "-lamdhip64", "-lm",
           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and "PASS" in out, out


def test_reynolds_sweep_example_runs(dev):
    """examples/ns2d_reynolds_sweep.py at a small size: the more viscous member ends with less enstrophy."""
    import os
    import subprocess
    import sys

    from conftest import ROOT

    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ns2d_reynolds_sweep.py"), "--n", "64", "--members", "3",
                        "--steps", "40"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    z = [float(line.split("enstrophy =")[1]) for line in out.splitlines() if "enstrophy =" in line]
    assert len(z) == 3 and z[0] < z[1] < z[2], out
