"""FNO3d baseline, everything that needs no GPU: the checkpoint contract (keys, shapes, dtypes, seeded initialisation) against
the reference's recorded tables, the plain-torch restatement tests/fno3d_ops.py against every golden case, the C ABI's answers
for the model's block shapes, and the loud refusals.

Tolerances (the project's own for an fp32 model against the reference): forward rel-L2 < 1e-5, gradients
|g - g_ref| < 5e-5 |g_ref| + 2e-9 per tensor.  Two correct CPU evaluations (reference, restatement) differ by up to 8.9e-7 /
1.9e-6 on these cases (printed by tests/golden/make_golden_fno3d.py)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import fno3d_ops as ops
from conftest import load_golden, rel_l2
from torch_cfd_amd import _lib
from torch_cfd_amd.fno import FNO3d, MLP

FWD_TOL = 1e-5


def grad_close(g, ref):
    g, ref = torch.as_tensor(g), torch.as_tensor(ref)
    if g.is_complex() or ref.is_complex():
        g, ref = torch.view_as_real(g.to(torch.complex128)), torch.view_as_real(ref.to(torch.complex128))
    g, ref = g.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    err, bound = torch.linalg.norm(g - ref).item(), 5e-5 * torch.linalg.norm(ref).item() + 2e-9
    return err, bound


def golden_state(case):
    g = load_golden(f"fno3d_{case}.npz")
    return g, {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd_")}


def test_state_dict_matches_recorded_tables():
    table = json.loads(str(load_golden("fno3d_state_tables.npz")["table"]))
    assert len(table) == 3
    for name, rec in table.items():
        sd = FNO3d(*rec["args"], **rec["kwargs"]).state_dict()
        got = [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]
        assert got == rec["state"], name


def test_attributes_kept():
    m = FNO3d(4, 3, 2, 8, input_channel=5, padding=2, channel_expansion=32, debug=True)
    assert (m.modes1, m.modes2, m.modes3, m.width, m.input_channel, m.padding, m.extra_mlp, m.channel_expansion, m.debug) == \
        (4, 3, 2, 8, 5, 2, True, 32, True)
    assert isinstance(m.q, MLP) and isinstance(m.q.activation, torch.nn.Identity)
    assert isinstance(FNO3d(4, 3, 2, 8, last_activation=True).q.activation, torch.nn.GELU)


@pytest.mark.parametrize("case", list(ops.CASES))
def test_golden_checkpoint_loads_strict(case):
    _, sd = golden_state(case)
    model = FNO3d(**ops.ctor_kwargs(case))
    result = model.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_seeded_initialisation_is_the_reference():
    g, sd = golden_state("tiny")
    if str(g["torch_version"]) != torch.__version__:
        pytest.skip(f"golden parameters were drawn by torch {g['torch_version']}, this is {torch.__version__}: "
                    "the generator streams of two builds need not agree")
    torch.manual_seed(ops.SEED)
    model = FNO3d(**ops.ctor_kwargs("tiny"))
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("case", list(ops.CASES))
def test_restatement_reproduces_golden(case):
    g, sd = golden_state(case)
    gg = load_golden(f"fno3d_{case}_grad.npz")
    kw = ops.ctor_kwargs(case)
    x, target = ops.case_input(case)
    y, gx, grads = ops.loss_and_grads(sd, x, target, kw["padding"], kw["last_activation"])
    err = rel_l2(y, g["y"])
    print(f"{case}: forward rel-L2 {err:.3e}")
    assert err < FWD_TOL
    for name, got in [("x", gx)] + list(grads.items()):
        e, bound = grad_close(got, gg[f"g_{name}"])
        print(f"{case}: grad {name}: {e:.3e} (bound {bound:.3e})")
        assert e < bound, name


def _layout_query(lib, has_l1, ci, cm, co, P, c1, c2, mode):
    dims = (ctypes.c_int * 6)()
    one = ctypes.c_void_p(1) if has_l1 else None       # only null / non-null of w1 matters in a query
    rc = lib.tcfd_fno_pointwise_bwd(None, None, None, None, None, one, None, None, None, None, None, None, 0, dims, 2, ci, cm, co,
                                    P, 8, 0, c1, c2, mode, 0, None)
    return rc, list(dims)


def test_library_answers_for_the_model_shapes():
    """The data-less layout query of the backward entry point needs no device (the occupancy figure it may add is optional:
    dims[5] stays 0 without one), so this part runs here."""
    _lib.build_library()
    lib = _lib.load()
    assert lib.tcfd_version() == _lib.ABI_VERSION
    P = 16 * 16 * 8
    for W in (10, 16, 20, 32):
        for c2 in (2, 0):                               # GELU / GELU and GELU / identity layer tails, with the skip convolution
            rc, dims = _layout_query(lib, True, W, W, W, P, 2, c2, 1)
            assert rc == 0, (W, c2, lib.tcfd_last_error())
            assert dims[4] == dims[0] * dims[1] + dims[2] * dims[3] > 0
        # the tail's forward keeps the pre-activation for a GELU output, nothing for the identity
        assert lib.tcfd_fno_pointwise_bwd_saved(W, W, W, P, 2, 2) == 2
        assert lib.tcfd_fno_pointwise_bwd_saved(W, W, W, P, 2, 0) == 0
        for E in (32, 64, 128):                         # head with last_activation: W -> E -> 1, GELU between
            rc, dims = _layout_query(lib, True, W, E, 1, P, 2, 0, 0)
            assert rc == 0, (W, E, lib.tcfd_last_error())
        rc, dims = _layout_query(lib, False, W, W, 1, P, 0, 0, 0)      # folded head: the W -> 1 reduction
        assert rc == 0
        for ci in (13, 8, 5, 2, 64):                    # lifting ci -> W
            if ci == W:
                continue
            rc, dims = _layout_query(lib, False, ci, ci, W, P, 0, 0, 0)
            assert rc == 0, (ci, W, lib.tcfd_last_error())
            assert dims[0] >= W and dims[1] >= ci + 1 and dims[4] == dims[0] * dims[1]
    rc, _ = _layout_query(lib, False, 13, 13, 11, P, 0, 0, 0)           # an odd width stays outside the family
    assert rc != 0 and b"not instantiated" in lib.tcfd_last_error()


def test_refusals():
    """Shape and precision are checked before the device, so all three refusals show without one."""
    model = FNO3d(4, 3, 3, 8, input_channel=5)
    with pytest.raises(_lib.TcfdError):
        model(torch.zeros(2, 8, 16, 16, 8))                             # a CPU tensor: no CPU fallback
    with pytest.raises(ValueError):
        model(torch.zeros(2, 7, 16, 16, 8))                             # input_channel + 3 = 8 channels expected
    with pytest.raises(TypeError):
        model(torch.zeros(2, 8, 16, 16, 8, dtype=torch.float64))        # float64 input
    with pytest.raises(TypeError):
        FNO3d(4, 3, 3, 8, input_channel=5).double()(torch.zeros(2, 8, 16, 16, 8))     # float64 model
    with pytest.raises(TypeError):
        FNO3d(4, 3, 3, 8, input_channel=5).double()(torch.zeros(2, 8, 16, 16, 8, dtype=torch.float64))
