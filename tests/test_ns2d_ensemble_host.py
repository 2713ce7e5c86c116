"""Host-side checks of ensembles with per-sample parameters: constructor parsing, buffers and ``state_dict``, the golden file's
self-consistency, the ABI symbol.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

L = 2 * math.pi
NU = (1e-3, 1e-2, 5e-2, 2e-1)
DRAG = (0.1, 0.0, 0.5, 0.05)
FSCALE = (1.0, 0.0, -2.0, 0.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


def make(viscosity, drag=0.0, **kw):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(16, 16), domain=((0, L), (0, L)))
    return tc.NavierStokes2DSpectral(viscosity, grid, drag=drag, solver=tc.RK4CrankNicolsonStepper(), **kw)


@pytest.mark.parametrize("real", [torch.float64, torch.float32])
def test_parameter_forms_give_the_same_operator(real):
    torch.set_default_dtype(real)
    a = make(list(NU), drag=list(DRAG), forcing_scale=list(FSCALE))
    b = make(torch.tensor(NU), drag=torch.tensor(DRAG), forcing_scale=torch.tensor(FSCALE))
    c = make(torch.tensor(NU).view(4, 1, 1), drag=torch.tensor(DRAG).view(4, 1, 1), forcing_scale=np.array(FSCALE))
    for op in (a, b, c):
        assert op._ens_count == 4
        for name, values in (("viscosity", NU), ("drag", DRAG), ("forcing_scale", FSCALE)):
            buf = getattr(op, name)
            assert buf.shape == (4, 1, 1) and buf.dtype == real
            assert torch.equal(buf.flatten(), torch.tensor(values, dtype=torch.float64).to(real))
    # the reference's value, evaluated on request: no resident table
    lin = a.linear_term
    assert lin.shape == (4, 16, 9) and lin.dtype == real
    assert torch.equal(lin, a.viscosity * a.laplace - a.drag)
    assert "linear_term" not in dict(a.named_buffers())
    for b_ in range(4):
        assert torch.equal(lin[b_], make(NU[b_], drag=DRAG[b_]).linear_term)      # member b's table is the scalar operator's


def test_single_values_are_repeated_and_defaults():
    torch.set_default_dtype(torch.float64)
    op = make(list(NU))                     # drag = 0, forcing_scale = 1
    assert torch.equal(op.drag.flatten(), torch.zeros(4)) and torch.equal(op.forcing_scale.flatten(), torch.ones(4))
    op = make(1e-3, drag=list(DRAG))        # a sequence anywhere makes the ensemble
    assert op._ens_count == 4 and torch.equal(op.viscosity.flatten(), torch.full((4,), 1e-3))
    op = make(1e-3, forcing_scale=[1.0, 2.0])
    assert op._ens_count == 2
    op = make(torch.tensor(1e-3), drag=torch.tensor(0.1))     # 0-dim tensors are single values: the scalar operator
    assert op._ens_count == 0


def test_mismatches_and_bad_shapes_raise():
    with pytest.raises(ValueError, match="viscosity has 4.*drag has 3"):
        make(list(NU), drag=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="forcing_scale has 2"):
        make(list(NU), forcing_scale=[1.0, 2.0])
    with pytest.raises(ValueError, match=r"\(2, 2\)"):
        make(torch.ones(2, 2))
    with pytest.raises(ValueError, match=r"\(4, 1\)"):
        make(torch.ones(4, 1))
    with pytest.raises(NotImplementedError, match="requires grad"):
        make(torch.tensor(NU, requires_grad=True))
    with pytest.raises(NotImplementedError, match="requires grad"):
        make(list(NU), drag=torch.tensor(0.1, requires_grad=True))


def test_state_dicts():
    torch.set_default_dtype(torch.float64)
    scalar = make(1e-3, drag=0.1)
    keys = [k for k in scalar.state_dict() if not k.startswith("solver.")]
    assert keys == ["kx", "ky", "laplace", "linear_term", "filter"]              # the reference's contract, untouched
    assert scalar.viscosity == 1e-3 and scalar.drag == 0.1 and scalar.forcing_scale is None and scalar._ens_count == 0
    ens = make(list(NU), drag=list(DRAG), forcing_scale=list(FSCALE))
    keys = [k for k in ens.state_dict() if not k.startswith("solver.")]
    assert keys == ["kx", "ky", "laplace", "viscosity", "drag", "forcing_scale", "filter"]
    sd = ens.state_dict()
    assert torch.equal(sd["viscosity"].flatten(), torch.tensor(NU)) and sd["drag"].shape == (4, 1, 1)
    import copy
    import pickle

    for other in (copy.deepcopy(ens), pickle.loads(pickle.dumps(ens))):      # plans are rebuilt lazily, the members travel
        assert other._ens_count == 4 and other._plans == {}
        assert torch.equal(other.linear_term, ens.linear_term) and torch.equal(other.forcing_scale, ens.forcing_scale)


def test_shapes_and_refusals_without_a_device():
    torch.set_default_dtype(torch.float64)
    op = make(list(NU), drag=list(DRAG))
    w = torch.randn(4, 16, 9, dtype=torch.complex128)
    assert torch.equal(op.implicit_terms(w), op.linear_term * w)
    w4 = torch.randn(4, 3, 16, 9, dtype=torch.complex128)
    assert torch.equal(op.implicit_solve(w4, 0.1), w4 / (1 - 0.1 * op.linear_term.unsqueeze(1)))
    for bad in (w[:3], w[0], w4[:2]):
        with pytest.raises(ValueError, match="B = 4"):
            op.implicit_terms(bad)
        with pytest.raises(ValueError, match="B = 4"):
            op(bad, 1e-3)
    for call in (lambda: op.tangent_step(w, w, 1e-3), lambda: op.explicit_terms_jvp(w, w), lambda: op.adjoint_step(w, w, 1e-3)):
        with pytest.raises(NotImplementedError, match="per-sample parameters"):
            call()


def test_data_generators_check_the_sequence_length():
    from torch_cfd_amd import data_gen

    assert data_gen._per_sample_values(4, viscosity=1e-3, drag=0.1, scale=torch.tensor(1.0)) == {}
    got = data_gen._per_sample_values(3, viscosity=[1e-3, 1e-2, 1e-1], drag=0.1)
    assert list(got) == ["viscosity"] and got["viscosity"].dtype == torch.float64
    with pytest.raises(ValueError, match="total_samples = 4"):
        data_gen._per_sample_values(4, viscosity=[1e-3, 1e-2])


def test_golden_file_is_self_consistent():
    g = load_golden("ns2d_ensemble.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ns2d_ensemble.npz")) < 1 << 20
    assert tuple(g["nu"]) == NU and tuple(g["drag"]) == DRAG and tuple(g["fscale"]) == FSCALE and float(g["dt"]) == 1e-3
    assert g["f64_w0"].shape == (4, 64, 33) and g["f64_w0"].dtype == np.complex128
    assert g["g32_w0"].shape == (4, 32, 17)
    for tag, cdt in (("f64", np.complex128), ("f32", np.complex64)):
        for key in ("F", "w1", "w10", "res1", "imex2"):
            a = g[f"{tag}_{key}"]
            assert a.shape == (4, 64, 33) and a.dtype == cdt and np.isfinite(a).all(), (tag, key)
        assert g[f"{tag}_g32_grad"].shape == (4, 32, 17) and g[f"{tag}_g32_grad"].dtype == cdt
        # the two precisions ran the same problem
        if tag == "f32":
            for key in ("F", "w1", "w10", "imex2"):
                d = np.linalg.norm(g[f"f32_{key}"] - g[f"f64_{key}"]) / np.linalg.norm(g[f"f64_{key}"])
                assert d < 1e-5, (key, d)
        # F in the rows the 2/3-rule mask removes is exactly zero
        F = g[f"{tag}_F"]
        assert np.all(F[:, 22:43, :] == 0) and np.any(F[:, :21, :] != 0)
    # every member moved, and differently: a member stepped with a neighbour's parameters is another flow
    w0, w10 = g["f64_w0"], g["f64_w10"]
    for b in range(4):
        assert np.linalg.norm(w10[b] - w0[b]) / np.linalg.norm(w0[b]) > 1e-3
    # the first-step states carry the viscosities: the high-wavenumber rows decay faster member by member
    decay = [np.linalg.norm(g["f64_w1"][b][20:22]) / np.linalg.norm(w0[b][20:22]) for b in range(4)]      # high-wavenumber rows
    assert decay[0] > decay[1] > decay[2] > decay[3]


def test_symbol_is_declared_exported_and_bound():
    import torch_cfd_amd as tc

    header = open(os.path.join(ROOT, "include", "tcfd.h")).read()
    decl = re.search(r"int tcfd_ns2d_plan_set_ensemble\(([^;]*)\);", header)
    assert decl and re.sub(r"\s+", " ", decl.group(1)) == ("tcfd_ns2d_plan* plan, long count, const double* laplace, const double* nu, "
                                                          "const double* drag, const double* forcing_scale")
    res, args = tc._lib.SIGNATURES["tcfd_ns2d_plan_set_ensemble"]
    assert len(args) == 6
    lib = tc._lib.load()
    assert hasattr(lib, "tcfd_ns2d_plan_set_ensemble")
    assert lib.tcfd_ns2d_plan_set_ensemble(None, 1, None, None, None, None) == -1          # TCFD_EINVAL, before any device call
    assert b"null plan" in lib.tcfd_last_error()
