"""CPU tests of the finite-volume advection schemes' host side: the scheme descriptors of torch_cfd_amd.interpolation / fvm,
the `convect` argument, the plan key, the ABI constants, and the plain-torch restatement tests/fvm_schemes_ops.py against the
reference's goldens tests/golden/fvm_schemes_<scheme>.npz (bounds: those of tests/test_fvm_host.py and
tests/test_fvm_grad_host.py for the same quantities)."""
import ctypes
import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch

import fvm_ops as F
import fvm_schemes_ops as S
from conftest import ROOT, load_golden, rel_l2

L = 2 * math.pi
STARTS = F.EDGE_STARTS + ("smooth",)


def _golden(scheme):
    return load_golden(f"fvm_schemes_{scheme}.npz")


def _pair(a):
    t = torch.from_numpy(np.asarray(a))
    return t[..., 0, :, :], t[..., 1, :, :]


def _leaves(a):
    return tuple(c.clone().requires_grad_() for c in _pair(a))


def _vjp(fn, u, cot):
    cx, cy = _pair(cot)
    out = fn(u)
    return torch.stack(torch.autograd.grad((out[0] * cx).sum() + (out[1] * cy).sum(), u))


def _physics(g, scheme):
    return S.Physics(scheme, int(g["n"]), nu=float(g["nu"]), drag=float(g["drag"]), wave=int(g["wave"]))


def _weights(method, dt):
    import torch_cfd_amd as tc

    return tc.RKStepper.from_method(method=method).weights(dt)


# ----------------------------------------------------------------------------- the goldens and the restatement
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_golden_inputs_are_the_shared_families(scheme):
    g = _golden(scheme)
    assert [str(s) for s in g["starts"]] == list(STARTS) and str(g["scheme"]) == scheme
    for si, name in enumerate(F.EDGE_STARTS):
        assert torch.equal(F.degenerate_start(name, int(g["n"]), seed=100 + si), torch.from_numpy(g[f"{name}_u0"]))
    for k in g.files:
        assert g[k].dtype.kind in "US" or np.isfinite(g[k]).all(), k


def test_van_leer_built_through_the_limiter_equals_the_default_convect():
    """apply_tvd_limiter(lax_wendroff, van_leer_limiter) handed to advect_general is the reference's own `convect`: its
    goldens on the degenerate starts are those of fvm_edges.npz, bit for bit."""
    g, e = _golden("van_leer"), load_golden("fvm_edges.npz")
    assert float(g["dt"]) == float(e["a1_dt"])
    for name in F.EDGE_STARTS:
        for what in ("explicit", "classic_rk4_1", "classic_rk4_3"):
            assert np.array_equal(g[f"{name}_{what}"], e[f"a1_{name}_{what}"]), (name, what)


def test_the_schemes_are_told_apart_by_the_bounds():
    """The explicit terms of the schemes differ by tens of per cent on the smooth start: a test at 1e-12 cannot pass with
    another scheme's kernel."""
    ref = _golden("upwind")["smooth_explicit"]
    for scheme in ("linear", "lax_wendroff", "van_leer"):
        assert rel_l2(_golden(scheme)["smooth_explicit"], ref) >= 0.1, scheme
    assert rel_l2(_golden("linear")["smooth_explicit"], _golden("lax_wendroff")["smooth_explicit"]) >= 1e-3


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_restatement_against_the_reference(scheme, start):
    g = _golden(scheme)
    ph, dt = _physics(g, scheme), float(g["dt"])
    u0 = _pair(g[f"{start}_u0"])
    assert rel_l2(torch.stack(ph.convect(dt)(u0)), g[f"{start}_convect"]) <= 1e-13
    assert rel_l2(torch.stack(ph.explicit(dt)(u0)), g[f"{start}_explicit"]) <= 1e-13
    a, b = _weights("classic_rk4", dt)
    assert rel_l2(torch.stack(ph.rollout(a, b, dt, 1)(u0)), g[f"{start}_classic_rk4_1"]) <= 1e-13
    assert rel_l2(torch.stack(ph.rollout(a, b, dt, 3)(u0)), g[f"{start}_classic_rk4_3"]) <= 1e-12


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("scheme", S.SCHEMES)
def test_restatement_gradients_against_the_reference(scheme, start):
    """Autograd through the restatement takes the reference's branches: w > 0 selects and passes no gradient."""
    g = _golden(scheme)
    ph, dt = _physics(g, scheme), float(g["dt"])
    cot = g[f"{start}_cot"]
    got = _vjp(ph.explicit(dt), _leaves(g[f"{start}_u0"]), cot)
    assert rel_l2(got, g[f"{start}_explicit_vjp"]) <= 1e-13
    a, b = _weights("forward_euler", dt)
    got = _vjp(ph.rollout(a, b, dt, 1), _leaves(g[f"{start}_u0"]), cot)
    assert rel_l2(got, g[f"{start}_forward_euler_vjp"]) <= 1e-12
    if start == "smooth":
        a, b = _weights("classic_rk4", dt)
        got = _vjp(ph.rollout(a, b, dt, 3), _leaves(g[f"{start}_u0"]), cot)
        assert rel_l2(got, g[f"{start}_classic_rk4_3_vjp"]) <= 1e-12


def test_restatement_leaves_fvm_ops_as_it_found_it():
    g = _golden("upwind")
    u0 = _pair(g["smooth_u0"])
    before = F.explicit_terms(u0[0], u0[1], 0.01, L / 16, 1e-3)
    S.explicit_terms("upwind", u0[0], u0[1], 0.01, L / 16, 1e-3)
    after = F.explicit_terms(u0[0], u0[1], 0.01, L / 16, 1e-3)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    same = S.explicit_terms("van_leer", u0[0], u0[1], 0.01, L / 16, 1e-3)
    assert torch.equal(before[0], same[0]) and torch.equal(before[1], same[1])


def test_fp32_restatement_within_the_fp32_bound():
    """The fp32 goldens (n = 64) against the restatement in fp32 torch ops: two fp32 pipelines, the bound of the GPU test."""
    for scheme in S.SCHEMES:
        g = _golden(scheme)
        ph = S.Physics(scheme, int(g["f32_n"]), nu=float(g["nu"]), drag=float(g["drag"]), wave=int(g["f32_wave"]))
        dt = float(g["f32_dt"])
        u0 = _pair(g["f32_v0"])
        assert u0[0].dtype == torch.float32
        a, b = _weights("classic_rk4", dt)
        out = ph.rollout(a, b, dt, 10, dtype=torch.float32)(u0)
        assert out[0].dtype == torch.float32
        assert rel_l2(torch.stack(out), g["f32_classic_rk4_10"]) <= 1e-5, scheme


# ----------------------------------------------------------------------------- descriptors
def test_descriptors_compare_and_hash_by_value():
    from torch_cfd_amd import fvm, interpolation as I

    a, b = fvm.advection(I.upwind), fvm.advection(I.upwind, I.linear)
    assert a == b and hash(a) == hash(b) and a is not b
    assert len({fvm.advection(c) for c in (I.upwind, I.linear, I.lax_wendroff, I.apply_tvd_limiter(I.lax_wendroff))}) == 4
    assert len({a, b, fvm.convect}) == 2
    assert I.upwind != I.linear and I.lax_wendroff != I.apply_tvd_limiter(I.lax_wendroff)
    assert repr(I.upwind) == "interpolation.upwind" and "lax_wendroff" in repr(fvm.convect) and "upwind" in repr(a)
    assert not isinstance(a, torch.nn.Module) and not isinstance(I.upwind, torch.nn.Module)
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.c_interpolation_fn = I.linear
    with pytest.raises(dataclasses.FrozenInstanceError):
        I.upwind.scheme = 0


def test_the_limited_lax_wendroff_is_the_default_convect():
    import torch_cfd_amd as tc
    from torch_cfd_amd import fvm, interpolation as I

    assert fvm.advection(I.apply_tvd_limiter(I.lax_wendroff)) == fvm.convect
    assert fvm.advection(I.apply_tvd_limiter(I.lax_wendroff, I.van_leer_limiter)) == fvm.convect
    assert fvm.advection(I.apply_tvd_limiter(I.lax_wendroff, limiter=I.van_leer_limiter), I.linear) == fvm.convect
    assert tc.advection is fvm.advection and tc.interpolation is I and tc.fvm is fvm


def test_unsupported_combinations_raise_naming_what_is_supported():
    from torch_cfd_amd import fvm, interpolation as I

    for bad in ((I.upwind,), (I.linear,), (I.lax_wendroff, I.linear), (I.lax_wendroff, torch.tanh)):
        with pytest.raises(NotImplementedError, match="lax_wendroff.*van_leer_limiter"):
            I.apply_tvd_limiter(*bad)
    with pytest.raises(NotImplementedError, match="linear"):
        fvm.advection(I.upwind, I.upwind)
    with pytest.raises(TypeError, match="upwind"):
        fvm.advection(lambda c, offset, v, dt: c)


def _grid(n=16):
    import torch_cfd_amd as tc

    return tc.Grid(shape=(n, n), domain=((0, L), (0, L)))


def test_a_foreign_callable_raises_type_error_listing_the_descriptors():
    import torch_cfd_amd as tc
    from torch_cfd_amd import interpolation as I

    def my_convect(v, dt):
        return v

    for bad in (my_convect, I.upwind, "upwind"):   # an interpolation is not a convect: fvm.advection(...) makes one
        with pytest.raises(TypeError) as e:
            tc.NavierStokes2DFVMProjection(1e-3, _grid(), convect=bad)
        msg = str(e.value)
        assert "cannot run in the HIP kernels" in msg
        for name in ("fvm.convect", "interpolation.upwind", "interpolation.linear", "interpolation.lax_wendroff",
                     "apply_tvd_limiter"):
            assert name in msg, name


def test_plan_key_differs_per_scheme_and_the_default_spellings_share_one():
    import torch_cfd_amd as tc
    from torch_cfd_amd import fvm, interpolation as I

    def key(**kw):
        """The key without the identity and version of the equation's own inverse-eigenvalue buffer."""
        k = tc.NavierStokes2DFVMProjection(1e-3, _grid(), drag=0.1, **kw)._plan_key(torch.float64, "cuda:0")
        assert len(k) == 10
        return k[:7] + k[9:]

    default = key()
    assert key(convect=None) == default and key(convect=fvm.convect) == default
    assert key(convect=fvm.advection(I.apply_tvd_limiter(I.lax_wendroff))) == default
    keys = {key(convect=fvm.advection(c)) for c in (I.upwind, I.linear, I.lax_wendroff)} | {default}
    assert len(keys) == 4
    eq = tc.NavierStokes2DFVMProjection(1e-3, _grid(), convect=fvm.advection(I.upwind))
    assert eq._plan_key(torch.float64, "cuda:0") != tc.NavierStokes2DFVMProjection(1e-3, _grid())._plan_key(torch.float64, "cuda:0")
    assert eq.advection == fvm.advection(I.upwind)


def test_state_dict_layout_is_unchanged_by_a_scheme():
    import torch_cfd_amd as tc
    from torch_cfd_amd import fvm, interpolation as I

    solver = lambda: tc.RKStepper.from_method(method="classic_rk4")   # noqa: E731
    a = tc.NavierStokes2DFVMProjection(1e-3, _grid(), solver=solver())
    b = tc.NavierStokes2DFVMProjection(1e-3, _grid(), solver=solver(), convect=fvm.advection(I.upwind))
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)


# ----------------------------------------------------------------------------- C ABI
def test_abi_constants_equal_the_header():
    import torch_cfd_amd as tc

    text = open(os.path.join(ROOT, "include", "tcfd.h")).read()
    for name in ("TCFD_FVM_VAN_LEER", "TCFD_FVM_UPWIND", "TCFD_FVM_LINEAR", "TCFD_FVM_LAX_WENDROFF"):
        m = re.search(name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == getattr(tc._lib, name), name
    assert tc._lib.TCFD_FVM_VAN_LEER == 0
    assert int(re.search(r"#define TCFD_ABI_VERSION (\d+)", text).group(1)) == tc._lib.ABI_VERSION == 13
    assert tc._lib.SIGNATURES["tcfd_fvm_plan_set_advection"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])


def test_an_unknown_scheme_is_an_invalid_argument_that_names_the_value():
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    rc = lib.tcfd_fvm_plan_set_advection(None, 7)   # the value is checked before the plan is touched
    assert rc == -1 and b"scheme 7" in lib.tcfd_last_error()
    rc = lib.tcfd_fvm_plan_set_advection(None, -1)
    assert rc == -1 and b"scheme -1" in lib.tcfd_last_error()
