"""Host-side checks of finite-volume ensembles (per-sample viscosity, drag and forcing amplitude of
``NavierStokes2DFVMProjection``): constructor parsing and its errors, the refusals that need no device, the golden file's
self-consistency, the ABI symbol.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

L = 2 * math.pi
NU = (1e-2, 3e-3, 1e-3, 3e-4)
DRAG = (0.0, 0.1, 0.2, 0.05)
FSCALE = (1.0, 1.0, 2.0, 0.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TCFD_EINVAL = -1


def make(viscosity, drag=0.0, forced=True, **kw):
    import torch_cfd_amd as tc

    grid = tc.Grid(shape=(16, 16), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=2, offsets=grid.cell_faces) if forced else None
    return tc.NavierStokes2DFVMProjection(viscosity, grid, drag=drag, forcing=forcing,
                                          solver=tc.RKStepper.from_method(method="classic_rk4"), **kw)


def test_parameter_forms_give_the_same_members():
    a = make(list(NU), drag=list(DRAG), forcing_scale=list(FSCALE))
    b = make(torch.tensor(NU, dtype=torch.float32), drag=torch.tensor(DRAG, dtype=torch.float32), forcing_scale=torch.tensor(FSCALE))
    c = make(torch.tensor(NU).view(4, 1, 1), drag=torch.tensor(DRAG, dtype=torch.float64).view(4, 1, 1), forcing_scale=np.array(FSCALE))
    for eq in (a, b, c):
        assert eq._ens_count == 4
        nu, drag, fs = eq._members()
        for buf in (eq.viscosity, eq.drag, eq.forcing_scale):
            assert buf.shape == (4, 1, 1) and buf.dtype == torch.float64
        assert drag == eq.drag.flatten().tolist() and fs == eq.forcing_scale.flatten().tolist()
        assert nu == eq.viscosity.flatten().tolist()       # density 1
    assert a._members() == (list(NU), list(DRAG), list(FSCALE))
    assert b._members()[0] == [float(np.float32(v)) for v in NU]       # a float32 tensor carries float32 values
    dense = make(list(NU), density=2.0)
    assert dense._members()[0] == [v / 2.0 for v in NU]                # nu / density, as the scalar plan forms it


def test_single_values_are_repeated_and_defaults():
    eq = make(list(NU))                               # drag = 0, forcing_scale = 1
    assert eq._members() == (list(NU), [0.0] * 4, [1.0] * 4)
    eq = make(1e-3, drag=list(DRAG))                  # a sequence anywhere makes the ensemble
    assert eq._ens_count == 4 and eq._members()[0] == [1e-3] * 4
    eq = make(1e-3, forcing_scale=[1.0, 2.0])
    assert eq._ens_count == 2 and eq._members()[2] == [1.0, 2.0]
    eq = make(list(NU), forced=False)                 # no forcing: no scales reach the plan
    assert eq._members()[2] is None
    for scalar in (make(1e-3, drag=0.1), make(torch.tensor(1e-3), drag=torch.tensor(0.1)), make(1e-3, forcing_scale=2.0)):
        assert scalar._ens_count == 0 and scalar._members() is None and "viscosity" not in dict(scalar.named_buffers())
    eq = make(1e-3, drag=0.1)
    assert eq.viscosity == 1e-3 and eq.drag == 0.1 and eq.forcing_scale is None      # the scalar attributes, as they were


def test_one_forcing_amplitude_scales_the_scalar_table():
    one, two = make(1e-3), make(1e-3, forcing_scale=2.0)
    for f1, f2 in zip(one._force_tables(), two._force_tables()):
        assert torch.equal(2.0 * f1, f2)
    assert one._plan_key(torch.float64, "cpu") != two._plan_key(torch.float64, "cpu")


def test_mismatches_and_bad_shapes_raise():
    with pytest.raises(ValueError, match="viscosity has 4.*drag has 3"):
        make(list(NU), drag=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="forcing_scale has 2"):
        make(list(NU), forcing_scale=[1.0, 2.0])
    with pytest.raises(ValueError, match=r"\(2, 2\)"):
        make(torch.ones(2, 2))
    with pytest.raises(ValueError, match=r"\(4, 1\)"):
        make(torch.ones(4, 1))
    with pytest.raises(ValueError, match="forcing_scale without a forcing"):
        make(list(NU), forced=False, forcing_scale=list(FSCALE))


def test_parameters_that_require_grad_are_refused():
    with pytest.raises(NotImplementedError, match="requires grad"):
        make(torch.tensor(NU, requires_grad=True))
    with pytest.raises(NotImplementedError, match="requires grad"):
        make(list(NU), drag=torch.tensor(0.1, requires_grad=True))
    with pytest.raises(NotImplementedError, match="requires grad"):
        make(list(NU), forcing_scale=torch.tensor(FSCALE, requires_grad=True))
    eq = make(list(NU))
    eq.viscosity.requires_grad_()           # a buffer turned into a leaf after construction: refused where the plan is made
    with pytest.raises(NotImplementedError, match="requires grad"):
        eq._plan_key(torch.float64, "cpu")


def test_a_batch_other_than_the_members_raises_before_any_device_call():
    eq = make(list(NU), drag=list(DRAG))
    good = torch.zeros(4, 16, 16, dtype=torch.float64)
    for bad in (good[:3], good[0], torch.zeros(5, 16, 16, dtype=torch.float64)):
        for call in (lambda u: eq((u, u), 1e-3), lambda u: eq.advance((u, u), 1e-3, steps=2), lambda u: eq.explicit_terms((u, u), 1e-3),
                     lambda u: eq.solver((u, u), 1e-3, eq), lambda u: eq.tangent_step((u, u), (u, u), 1e-3),
                     lambda u: eq.explicit_terms_jvp((u, u), (u, u), 1e-3)):
            with pytest.raises(ValueError, match="B = 4"):
                call(bad)


def test_the_plan_key_holds_the_member_values():
    eq = make(list(NU), drag=list(DRAG))
    key = eq._plan_key(torch.float64, "cpu")
    assert key == eq._plan_key(torch.float64, "cpu")
    eq.drag[1] = 0.3                                     # an in-place write
    changed = eq._plan_key(torch.float64, "cpu")
    assert changed != key
    eq.viscosity = eq.viscosity.clone()                  # another buffer
    assert eq._plan_key(torch.float64, "cpu") != changed
    import copy

    other = copy.deepcopy(eq)                            # plans are rebuilt lazily, the members travel
    assert other._ens_count == 4 and other._plans == {} and other._members() == eq._members()
    assert [k for k in eq.state_dict() if k in ("viscosity", "drag", "forcing_scale")] == ["viscosity", "drag", "forcing_scale"]


def test_golden_file_is_self_consistent():
    g = load_golden("fvm_ensemble.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fvm_ensemble.npz")) < 1 << 20
    assert tuple(g["nu"]) == NU and tuple(g["drag"]) == DRAG and tuple(g["scale"]) == FSCALE
    assert int(g["n"]) == 16 and float(g["dt"]) == 0.25 * L / 16 and float(g["tolerance"]) == 1e-11
    for key in ("u0", "du", "steps_1", "steps_5", "tangent_1"):
        assert g[key].shape == (4, 2, 16, 16) and g[key].dtype == np.float64 and np.isfinite(g[key]).all(), key
    # a member stepped with a neighbour's viscosity, drag or forcing scale is another flow, by far more than the test's tolerance
    for name in ("nu", "drag", "scale"):
        assert float(g[f"margin_{name}"]) >= 100 * float(g["tolerance"]), name
    for b in range(4):
        assert np.linalg.norm(g["steps_5"][b] - g["u0"][b]) / np.linalg.norm(g["u0"][b]) > 1e-3


def test_symbol_is_declared_exported_and_bound():
    import ctypes

    import torch_cfd_amd as tc

    header = open(os.path.join(ROOT, "include", "tcfd.h")).read()
    decl = re.search(r"int tcfd_fvm_plan_set_ensemble\(([^;]*)\);", header)
    assert decl and re.sub(r"\s+", " ", decl.group(1)) == ("tcfd_fvm_plan* plan, long count, const double* nu_over_density, "
                                                          "const double* drag, const double* forcing_scale")
    res, args = tc._lib.SIGNATURES["tcfd_fvm_plan_set_ensemble"]
    dp = ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_long, dp, dp, dp]
    lib = tc._lib.load()
    assert hasattr(lib, "tcfd_fvm_plan_set_ensemble") and lib.tcfd_fvm_plan_set_ensemble.argtypes == args
    nu = tc._lib.darray(NU)
    assert lib.tcfd_fvm_plan_set_ensemble(None, 4, nu, None, None) == TCFD_EINVAL          # before any device call
    assert b"null plan" in lib.tcfd_last_error()
    assert lib.tcfd_fvm_plan_set_ensemble(None, 0, None, None, None) == TCFD_EINVAL
