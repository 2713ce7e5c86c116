"""FNO3d baseline on the GPU: the model against the reference's recorded outputs and gradients, against the plain-torch
restatement (tests/fno3d_ops.py) at sizes too big for a fixture, each new kernel alone against torch ops, and the properties the
feature promises -- no torch fallback for the listed widths, no (b, E, P) hidden tensor in the head, bit-equal reruns.

Tolerances are the project's own, none is new: an fp32 model against the reference  forward rel-L2 < 1e-5
(test_sfno_tiny_end_to_end_golden), gradients |g - g_ref| < 5e-5 |g_ref| + 2e-9 per tensor (test_sfno_training_step_gradients_golden);
a fused kernel against the composed torch ops  2e-6 (outputs, test_fused_pointwise_block_matches_torch_modules) and 2e-5
(gradients, test_pointwise_backward_kernel_matches_autograd)."""
import pytest
import torch
import torch.nn as nn

import fno3d_ops as ops
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
FUSED_OUT, FUSED_GRAD = 2e-6, 2e-5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def grad_err(g, ref):
    g, ref = torch.as_tensor(g), torch.as_tensor(ref)
    if g.is_complex() or ref.is_complex():
        g, ref = torch.view_as_real(g.to(torch.complex128)), torch.view_as_real(ref.to(torch.complex128))
    g, ref = g.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return torch.linalg.norm(g - ref).item(), 5e-5 * torch.linalg.norm(ref).item() + 2e-9


def model_loss_grads(model, x, target):
    """(y, second output, gradient of mean((y - target)^2) w.r.t. the input, {parameter name: gradient})."""
    x = x.detach().clone().requires_grad_(True)
    y, second = model(x)
    loss = ((y - target) ** 2).mean()
    named = list(model.named_parameters())
    grads = torch.autograd.grad(loss, [x] + [p for _, p in named])
    return y.detach(), second, grads[0], {n: g for (n, _), g in zip(named, grads[1:])}


def assert_matches(tag, y, gx, grads, y_ref, gx_ref, grads_ref):
    err = rel_l2(y, y_ref)
    print(f"{tag}: forward rel-L2 {err:.3e}")
    worst = []
    for name, got, ref in [("x", gx, gx_ref)] + [(n, grads[n], grads_ref[n]) for n in grads_ref]:
        e, bound = grad_err(got, ref)
        print(f"{tag}: grad {name}: {e:.3e} (bound {bound:.3e})")
        if not e < bound:
            worst.append((name, e, bound))
    assert err < FWD_TOL, (tag, err)
    assert not worst, (tag, worst)


# ----------------------------------------------------------------------------- 5. golden cases
@pytest.mark.parametrize("case", list(ops.CASES))
def test_golden_case(case, dev):
    from torch_cfd_amd.fno import FNO3d

    g, gg = load_golden(f"fno3d_{case}.npz"), load_golden(f"fno3d_{case}_grad.npz")
    model = FNO3d(**ops.ctor_kwargs(case))
    model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd_")}, strict=True)
    model = model.to(dev)
    x, target = ops.case_input(case)
    y, second, gx, grads = model_loss_grads(model, x.to(dev), target.to(dev))
    assert second is None and y.shape == target.shape
    with torch.no_grad():                                   # the forward-only path (other kernels for p, the layers and q)
        y0, second0 = model(x.to(dev))
    assert second0 is None and rel_l2(y0, g["y"]) < FWD_TOL
    assert_matches(case, y, gx, grads, g["y"], gg["g_x"], {n: gg[f"g_{n}"] for n in grads})


# ----------------------------------------------------------------------------- 6. / 11. against the restatement on the same GPU
def against_restatement(tag, dev, args, kw, shape, seed=3):
    from torch_cfd_amd.fno import FNO3d

    torch.manual_seed(seed)
    model = FNO3d(*args, **kw).to(dev)
    x = torch.randn(*shape, device=dev)
    target = torch.randn(shape[0], *shape[2:], device=dev)
    y, second, gx, grads = model_loss_grads(model, x, target)
    assert second is None
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    y_ref, gx_ref, grads_ref = ops.loss_and_grads(sd, x, target, kw.get("padding", 0), kw.get("last_activation", False))
    assert_matches(tag, y, gx, grads, y_ref, gx_ref, grads_ref)


def test_notebook_size_against_restatement(dev):
    against_restatement("notebook", dev, (32, 32, 5, 10), {"input_channel": 10}, (4, 13, 64, 64, 10))


def test_wide_against_restatement(dev):
    against_restatement("wide", dev, (12, 12, 5, 20), {}, (2, 13, 128, 128, 10))


@pytest.mark.parametrize("padding", [4, 3])
def test_padding_against_restatement(padding, dev):
    """24^2 + 2 x 4 = 32^2 runs the FFT kernels, 24^2 + 2 x 3 = 30^2 whatever ``_library_takes`` sends that size to."""
    against_restatement(f"padding{padding}", dev, (4, 4, 3, 8), {"input_channel": 5, "padding": padding, "num_spectral_layers": 2},
                        (2, 8, 24, 24, 8))


# ----------------------------------------------------------------------------- 7. each new kernel alone
def block_against_float64(dev, lin1, a1, lin2, skc, a2, shape, need_dx=True, expect_kernel=True, monkeypatch=None):
    """``hip_pointwise`` of one block, forward and backward, against the same block written with einsums in float64."""
    from torch_cfd_amd import fno

    two = lin1 is not None
    x = torch.randn(*shape, device=dev, requires_grad=need_dx)
    s = torch.randn(*shape, device=dev, requires_grad=True) if skc is not None else None
    with torch.no_grad():
        out0 = fno.hip_pointwise(x, lin1, a1, lin2, skip=s, skip_conv=skc, act2=a2)
    out = fno.hip_pointwise(x, lin1, a1, lin2, skip=s, skip_conv=skc, act2=a2)
    assert out0 is not None and out is not None and out.grad_fn is not None
    t = torch.randn_like(out)
    if expect_kernel and monkeypatch is not None:
        def no_fallback(*a_, **k_):
            raise AssertionError("fell back to the einsum recompute")
        monkeypatch.setattr(fno, "_pointwise_reference", no_fallback)
    (out * t).sum().backward()
    if monkeypatch is not None:
        monkeypatch.undo()
    d = lambda v: v.detach().double().requires_grad_(True) if v is not None else None
    leaves = [d(x), d(s), d(lin1.weight) if two else None, d(lin1.bias) if two else None, d(lin2.weight), d(lin2.bias),
              d(skc.weight) if skc else None, d(skc.bias) if skc else None, None, None]
    ref_out = fno._pointwise_reference((two, a1, a2, 1 if skc is not None else 0, None), *leaves)
    e0, e1 = rel_l2(out0, ref_out), rel_l2(out, ref_out)
    print(f"forward rel-L2 {e0:.3e} (no grad) {e1:.3e} (grad)")
    assert e0 < FUSED_OUT and e1 < FUSED_OUT
    (ref_out * t.double()).sum().backward()
    pairs = [("x", x.grad, leaves[0].grad)] if need_dx else []
    if s is not None:
        pairs.append(("s", s.grad, leaves[1].grad))
    for name, m, iw, ib in (("lin1", lin1, 2, 3), ("lin2", lin2, 4, 5), ("skip", skc, 6, 7)):
        if m is not None:
            pairs += [(name + ".w", m.weight.grad, leaves[iw].grad), (name + ".b", m.bias.grad, leaves[ib].grad)]
    for name, got, ref in pairs:
        if ref is not None:
            e = rel_l2(got, ref)
            print(f"grad {name}: rel-L2 {e:.3e}")
            assert got is not None and e < FUSED_GRAD, name
    if not need_dx:
        assert x.grad is None


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("W", [10, 20])
@pytest.mark.parametrize("ci", [13, 8, 5])
def test_lifting_kernel(ci, W, need_dx, dev, monkeypatch):
    torch.manual_seed(ci * 100 + W)
    block_against_float64(dev, None, None, nn.Conv3d(ci, W, 1).to(dev), None, None, (3, ci, 6, 8, 10), need_dx=need_dx,
                          monkeypatch=monkeypatch)


@pytest.mark.parametrize("shape", [(2, 13, 5, 7, 9), (2, 13, 6, 6, 7)])
def test_lifting_kernel_ragged(shape, dev, monkeypatch):
    """P % 4 != 0 (5 x 7 x 9 = 315 points) and an odd T with P % 4 == 0 ... 6 x 6 x 7 = 252: the guarded 4-byte paths."""
    torch.manual_seed(5)
    block_against_float64(dev, None, None, nn.Conv3d(13, 10, 1).to(dev), None, None, shape, need_dx=True, monkeypatch=monkeypatch)


@pytest.mark.parametrize("act2", ["GELU", None])
@pytest.mark.parametrize("W", [10, 16, 20, 32])
def test_layer_tail_backward_kernel(W, act2, dev, monkeypatch):
    """W -> W -> W with the skip convolution, GELU inside, GELU / identity outside (the FNO3d layer and its last layer)."""
    torch.manual_seed(W)
    a2 = getattr(nn, act2)() if act2 else nn.Identity()
    block_against_float64(dev, nn.Conv3d(W, W, 1).to(dev), nn.GELU(), nn.Conv3d(W, W, 1).to(dev), nn.Conv3d(W, W, 1).to(dev), a2,
                          (3, W, 6, 9, 10), monkeypatch=monkeypatch)


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("E", [32, 64, 128])
@pytest.mark.parametrize("W", [10, 20])
def test_head_kernels(W, E, gelu, dev, monkeypatch):
    """The head W -> E -> 1 through ``MLP``: folded (identity between) or the head kernels (GELU between), against the two
    convolutions evaluated one after the other in float64."""
    from torch_cfd_amd import fno

    torch.manual_seed(W + E)
    head = fno.MLP(W, 1, E, activation=gelu).to(dev)
    x = torch.randn(3, W, 6, 8, 10, device=dev, requires_grad=True)
    with torch.no_grad():
        out0 = head(x)

    def no_fallback(*a_, **k_):
        raise AssertionError("the head fell back to torch modules / the einsum recompute")
    monkeypatch.setattr(fno, "_pointwise_reference", no_fallback)
    monkeypatch.setattr(fno, "_note_torch_modules", no_fallback)
    out = head(x)
    t = torch.randn_like(out)
    (out * t).sum().backward()
    monkeypatch.undo()
    ref_head = fno.MLP(W, 1, E, activation=gelu).double().to(dev)
    ref_head.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    xd = x.detach().double().requires_grad_(True)
    ref = ref_head.mlp2(ref_head.activation(ref_head.mlp1(xd)))
    (ref * t.double()).sum().backward()
    e0, e1 = rel_l2(out0, ref), rel_l2(out, ref)
    print(f"forward rel-L2 {e0:.3e} (no grad) {e1:.3e} (grad)")
    assert e0 < FUSED_OUT and e1 < FUSED_OUT
    for (name, prm), (_, rp) in zip([("x", x)] + list(head.named_parameters()), [("x", xd)] + list(ref_head.named_parameters())):
        e = rel_l2(prm.grad, rp.grad)
        print(f"grad {name}: rel-L2 {e:.3e}")
        assert e < FUSED_GRAD, name


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("shape", [(2, 10, 5, 7, 9), (2, 10, 6, 6, 7)])
def test_head_ragged(shape, gelu, dev):
    """P % 4 != 0 and an odd T: results right, whatever path they take."""
    from torch_cfd_amd import fno

    torch.manual_seed(9)
    head = fno.MLP(10, 1, 64, activation=gelu).to(dev)
    x = torch.randn(*shape, device=dev, requires_grad=True)
    out = head(x)
    t = torch.randn_like(out)
    (out * t).sum().backward()
    ref_head = fno.MLP(10, 1, 64, activation=gelu).double().to(dev)
    ref_head.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    xd = x.detach().double().requires_grad_(True)
    ref = ref_head.mlp2(ref_head.activation(ref_head.mlp1(xd)))
    (ref * t.double()).sum().backward()
    assert rel_l2(out, ref) < FUSED_OUT
    for (name, prm), (_, rp) in zip([("x", x)] + list(head.named_parameters()), [("x", xd)] + list(ref_head.named_parameters())):
        assert rel_l2(prm.grad, rp.grad) < FUSED_GRAD, name


# ----------------------------------------------------------------------------- 8. no fallback
@pytest.mark.parametrize("last_activation", [False, True])
@pytest.mark.parametrize("args,kw,shape", [
    ((32, 32, 5, 10), {"input_channel": 10}, (4, 13, 64, 64, 10)),
    ((4, 4, 3, 16), {"input_channel": 10, "num_spectral_layers": 2}, (2, 13, 16, 16, 8)),
    ((4, 4, 3, 20), {"input_channel": 10, "num_spectral_layers": 2}, (2, 13, 16, 16, 8)),
    ((4, 4, 3, 32), {"input_channel": 10, "num_spectral_layers": 2}, (2, 13, 16, 16, 8)),
])
def test_no_torch_fallback(args, kw, shape, last_activation, dev, monkeypatch):
    """Forward + backward with the einsum recompute and the torch-module note turned into errors (the warning itself is issued
    once per process per shape, so turning warnings into errors would not be enough)."""
    from torch_cfd_amd import fno

    def refuse(*a_, **k_):
        raise AssertionError(f"FNO3d{args} fell off the HIP kernels: {a_[:1]}")
    monkeypatch.setattr(fno, "_pointwise_reference", refuse)
    monkeypatch.setattr(fno, "_note_torch_modules", refuse)
    torch.manual_seed(1)
    model = fno.FNO3d(*args, last_activation=last_activation, **kw).to(dev)
    x = torch.randn(*shape, device=dev)
    with torch.no_grad():
        y0, _ = model(x)
    y, _ = model(x)
    y.square().mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).all()
               for p in model.parameters())
    assert rel_l2(y0, y) < FUSED_OUT


# ----------------------------------------------------------------------------- 9. the head's hidden tensor never exists
@pytest.mark.parametrize("gelu", [False, True])
def test_head_never_forms_the_hidden_tensor(gelu, dev):
    from torch_cfd_amd import fno

    W, E, b, mesh = 10, 128, 4, (64, 64, 256)               # b P = 2^22 points
    points = b * mesh[0] * mesh[1] * mesh[2]
    assert points == 1 << 22
    torch.manual_seed(0)
    head = fno.MLP(W, 1, E, activation=gelu).to(dev)
    x = torch.randn(b, W, *mesh, device=dev, requires_grad=True)
    t = torch.randn(b, 1, *mesh, device=dev)
    for _ in range(2):                                      # first round: plans, lazily built tables, the allocator's pools
        head.zero_grad(set_to_none=True)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        out = head(x)
        (out * t).sum().backward()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - live
        del out
    hidden = points * E * 4
    print(f"head gelu={gelu}: peak rise {rise / 2**20:.0f} MiB over the live inputs, hidden tensor would be {hidden / 2**20:.0f} MiB")
    assert rise < hidden


# ----------------------------------------------------------------------------- 10. determinism
def test_backward_is_deterministic(dev):
    from torch_cfd_amd.fno import FNO3d

    torch.manual_seed(2)
    model = FNO3d(8, 8, 4, 10, input_channel=10, num_spectral_layers=2, last_activation=True).to(dev)
    x = torch.randn(2, 13, 32, 32, 10, device=dev)
    target = torch.randn(2, 32, 32, 10, device=dev)
    _, _, gx1, g1 = model_loss_grads(model, x, target)
    _, _, gx2, g2 = model_loss_grads(model, x, target)
    assert torch.equal(gx1, gx2)
    for n in g1:
        a, b_ = g1[n], g2[n]
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b_) if b_.is_complex() else b_), n
