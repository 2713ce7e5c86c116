#!/usr/bin/env python
"""Generate tests/golden/losses.npz by IMPORTING THE REFERENCE's fno/losses.py (CPU only, deterministic).

Run only where the reference checkout is present (read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py

Inputs are the seeded CPU draws of tests/losses_ops.py, which the tests draw again; only the reference's outputs (values,
gradients, tables) are stored.  ``BochnerNorm``'s constructor cannot be called in the reference (it hands ``time_last=`` to a
parent that has no such parameter), so the instance is made with ``__new__`` + ``nn.Module.__init__``, given the attributes its
forward reads, and the reference's forward is called.  Beside each float32 residual case the reference's own
float32-versus-float64 deviation is stored.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import losses_ops as ops  # noqa: E402
from fno import losses as ref  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


def grads(loss, *xs):
    return [npy(g) for g in torch.autograd.grad(loss, xs)]


def gen_residual(out):
    torch.set_default_dtype(torch.float64)
    for b, n, nt in ops.RESIDUAL_SHAPES:
        tag = f"res_{b}_{n}_{nt}"
        w, f, psi = ops.residual_inputs(b, n, nt)
        kw = dict(batch_size=b, visc=ops.residual_visc(n), n_grid=n, n_t=nt, delta_t=ops.RESIDUAL_DELTA_T)
        for norm in ("ortho", "backward", "forward"):
            m = ref.ResidualLoss(norm=norm, **kw)
            out[f"{tag}_{norm}_f"] = npy(m(w, f=f))
            out[f"{tag}_{norm}_nof"] = npy(m(w))
            out[f"{tag}_{norm}_psi"] = npy(m(w, psi=psi, f=f))
        m = ref.ResidualLoss(**kw)
        if n == 16 and nt == 5:
            out[f"{tag}_kx"], out[f"{tag}_ky"], out[f"{tag}_kt"], out[f"{tag}_lap"] = (npy(z[0]) for z in (m.kx, m.ky, m.kt, m.lap))
        if n <= 32:
            wr, fr, pr = (z.clone().requires_grad_(True) for z in (w, f, psi))
            gw, gf = grads(m(wr, f=fr), wr, fr)
            out[f"{tag}_gw"] = gw
            if n == 16:
                out[f"{tag}_gf"] = gf
            if (n, nt) == (16, 5):
                (out[f"{tag}_nof_gw"],) = grads(m(wr), wr)
                out[f"{tag}_psi_gw"], out[f"{tag}_psi_gpsi"] = grads(m(wr, psi=pr, f=fr), wr, pr)
        # the reference in float32 (module built under a float32 default) and its deviation from its own float64 result
        torch.set_default_dtype(torch.float32)
        m32 = ref.ResidualLoss(**kw)
        torch.set_default_dtype(torch.float64)
        w32, f32 = (z.float().requires_grad_(True) for z in (w, f))
        l32 = m32(w32, f=f32)
        out[f"{tag}_f32"] = npy(l32)
        ref64 = float(out[f"{tag}_ortho_f"])
        out[f"{tag}_f32_dev"] = np.array(abs(float(l32) - ref64) / abs(ref64))
        if n <= 32:
            g32 = grads(l32, w32)[0]
            out[f"{tag}_f32_gw_dev"] = np.array(ops.relerr(torch.from_numpy(g32), torch.from_numpy(out[f"{tag}_gw"])))
        if (n, nt) == (16, 5):
            out[f"{tag}_lap_f32"] = npy(m32.lap[0])
            out[f"{tag}_kt_f32"] = npy(m32.kt[0])
            # the float32-built module on float64 data (torch promotes: float32-rounded tables, float64 arithmetic)
            out[f"{tag}_mixed"] = npy(m32(w, f=f))


def gen_small(out):
    torch.set_default_dtype(torch.float64)
    x, y = ops.small_inputs(ops.SMALL_SHAPE_CH, 7)
    for name, kw in ops.LP_CASES.items():
        xr = x.clone().requires_grad_(True)
        val = ref.LpLoss(**kw)(xr, y)
        out[f"lp_{name}"] = npy(val)
        if name in ops.LP_GRAD_CASES:
            (out[f"lp_{name}_gx"],) = grads(val.sum(), xr)
    x17, y17 = ops.small_inputs((3, 2, 17, 17), 8)
    out["lp_odd_p3_rel"] = npy(ref.LpLoss(p=3, relative=True)(x17, y17))
    out["lp_odd_p2_abs"] = npy(ref.LpLoss(p=2)(x17, y17))
    for name, kw in ops.L2_CASES.items():
        preds, targets, tg, K = ops.l2_case_inputs(kw["kmode"])
        pr = preds.clone().requires_grad_(True)
        m = ref.L2Loss2d(metric_reduction=kw["metric_reduction"], weighted=kw["weighted"])
        val = m(pr, targets, targets_grad=tg if kw["with_grad"] else None, K=K)
        out[f"l2_{name}"] = npy(val)
        if name in ops.L2_GRAD_CASES:
            (out[f"l2_{name}_gp"],) = grads(val, pr)
    gx, gy = ref.central_diff(x)
    out["cd_gx"], out["cd_gy"] = npy(gx), npy(gy)
    (u,) = ops.small_inputs(ops.SMALL_SHAPE_TL, 9, 1)
    for name, kw in ops.BOCHNER_CASES.items():
        m = ref.BochnerNorm.__new__(ref.BochnerNorm)
        nn.Module.__init__(m)
        m.n_grid, m.mesh_weighted, m.reduction = ops.SMALL_SHAPE_TL[1], True, True
        m.time_last, m.p, m.dt, m.time_average = kw["time_last"], kw["p"], kw["dt"], kw["time_average"]
        ur = (u if kw["time_last"] else u.permute(0, 3, 1, 2).contiguous()).clone().requires_grad_(True)
        val = m(ur)
        out[f"bochner_{name}"] = npy(val)
        if name in ops.BOCHNER_GRAD_CASES:
            (out[f"bochner_{name}_gu"],) = grads(val, ur)


if __name__ == "__main__":
    out = {}
    gen_residual(out)
    gen_small(out)
    path = os.path.join(HERE, "losses.npz")
    np.savez_compressed(path, **out)
    print(f"losses.npz: {os.path.getsize(path)/1024:.1f} KiB, {len(out)} arrays")
