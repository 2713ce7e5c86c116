"""Helpers of the cotangent-bundle tests (tests/test_ns2d_cobundle_host.py, tests/test_ns2d_cobundle_gpu.py): the reverse-mode
reference of a bundle and seeded bundles of white-noise cotangents."""
import functools

import torch

import ns2d_bundle_ops as BO
import ns2d_ops

CPLX = BO.CPLX


def oracle_cobundle(fn, w, G):
    """``(fn(w), [(d fn / d w)^T G[k]])`` for a bundle ``G`` = (K,) + w.shape by torch autograd in the real inner product: ONE
    forward evaluation, the graph reversed once per cotangent.  ``fn`` maps (batch, n, m) to (batch, n, m)."""
    x = w.clone().requires_grad_(True)
    out = fn(x)
    grads = [torch.autograd.grad(ns2d_ops.real_inner(G[k], out), x, retain_graph=True)[0] for k in range(G.shape[0])]
    return out.detach(), torch.stack(grads)


@functools.lru_cache(maxsize=None)
def inputs(n, tag, B, K):
    """(w0, G) on the CPU in the precision of ``tag``: the B smooth vorticity fields of the tangent-bundle tests and K x B
    distinct white-noise complex cotangents of different amplitudes (they reach every wavenumber the mask keeps)."""
    w0, _ = BO.inputs(n, tag, B, 1)
    gen = torch.Generator().manual_seed(7000 + 31 * n + 7 * B + K)
    G = torch.view_as_complex(torch.randn(K, B, n, n // 2 + 1, 2, generator=gen, dtype=torch.float64))
    G = G * (0.5 + 0.25 * torch.arange(K, dtype=torch.float64))[:, None, None, None]
    return w0, G.to(CPLX[tag]).contiguous()


def row_launches(plan, fn, max_records=4096):
    """How many row-pass launches ``fn()`` makes on ``plan``, by the library's per-launch records (kind 1; the column passes are
    kinds 0, 2, 3 and 5).  One ``explicit_terms_vjp_bundle`` call on ONE state makes one per cotangent group with
    ``k_rows_vjp_bundle`` and one per cotangent with the out-of-place fall-back."""
    import ctypes

    from torch_cfd_amd import _lib

    lib = plan.lib
    cnt, kinds, ms = ctypes.c_int(0), (ctypes.c_int * max_records)(), (ctypes.c_float * max_records)()
    _lib.check(lib.tcfd_ns2d_profile_begin(plan.handle, max_records), "tcfd_ns2d_profile_begin")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.tcfd_ns2d_profile_end(plan.handle, max_records, ctypes.byref(cnt), kinds, ms), "tcfd_ns2d_profile_end")
    assert cnt.value < max_records
    return sum(1 for i in range(cnt.value) if kinds[i] == 1)


def pre_weighted(op, plan, G):
    """gm = mask * g / c of ``tcfd_ns2d_explicit_terms_vjp``: the cotangents times the ``pre`` table of the package."""
    from torch_cfd_amd import autograd as ad

    pre, post = ad.FusedExplicitTerms._tables(op, plan, G.device)
    return (G * pre).contiguous(), post
