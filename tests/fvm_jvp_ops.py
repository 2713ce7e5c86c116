"""Forward-mode helpers the tangent tests of the finite-volume solver share (test-only): dual numbers of
torch.autograd.forward_ad through a function of the velocity pair -- the restatement tests/fvm_ops.py /
tests/fvm_schemes_ops.py, or the package itself -- and the layout of tests/golden/fvm_jvp.npz."""
import torch
import torch.autograd.forward_ad as fwAD

METHODS = ("forward_euler", "midpoint", "heun_rk2", "classic_rk4")
CASES = ("n16_b2", "n32_b1")


def pair(a, device="cpu", dtype=torch.float64):
    """(..., 2, n, n) array of a golden -> the pair (ux, uy) of (..., n, n) tensors."""
    t = torch.as_tensor(a).to(device, dtype)
    return t[..., 0, :, :].contiguous(), t[..., 1, :, :].contiguous()


def stacked(p):
    """The pair back in a golden's layout, on the CPU."""
    return torch.stack([c.detach().cpu() for c in p], dim=-3)


def jvp(fn, u, du):
    """(fn(u), d fn(u) . du) by dual numbers: `fn` maps a pair (ux, uy) to a pair; a result without a tangent counts as zero."""
    with fwAD.dual_level():
        out = fn(tuple(fwAD.make_dual(a, d) for a, d in zip(u, du)))
        parts = [fwAD.unpack_dual(o) for o in out]
        primal = tuple(p.primal.detach().clone() for p in parts)
        tangent = tuple(torch.zeros_like(p.primal) if p.tangent is None else p.tangent.detach().clone() for p in parts)
    return primal, tangent


def perturbation(shape, seed, device="cpu", dtype=torch.float64):
    """A seeded (..., 2, n, n) perturbation as a pair."""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return pair(t, device, dtype)
