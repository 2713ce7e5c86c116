"""Reverse mode of the finite-volume solver (``fvm.py``): ``torch.autograd.Function``s over the adjoint kernels of
``csrc/tcfd_fvm.hip`` (C ABI ``tcfd_fvm_explicit_terms_vjp`` / ``tcfd_fvm_step_vjp``).

They engage only when grad mode is on and a velocity component requires grad; otherwise ``fvm.py`` runs its forward
kernels as before.  With stage weights ``A_ij = dt a_ij``, ``B_j = dt b_j`` one step is

    u_0 = u0,   u_i = P(u0 + sum_{j<i} A_ij k_j),   k_i = F(u_i),   u_new = P(u0 + sum_j B_j k_j)

and its reverse, given the cotangent ``ubar`` of ``u_new`` (``P`` is symmetric, so its VJP is ``P`` itself):

    mu = P ubar;  u0bar = mu;  kbar_j = B_j mu
    for i = s-1 .. 0:  g_i = J_F(u_i)^T kbar_i;  i = 0: u0bar += g_0;  i > 0: mu_i = P g_i;  u0bar += mu_i;  kbar_j += A_ij mu_i

``StepFn`` keeps the input of every step and recomputes the stage states in the backward: a rollout of K steps holds
``K * 2 * B * n^2 * w`` bytes (``w`` = 8 for fp64, 4 for fp32) until its backward has run, plus the plan's workspace
(``tcfd_fvm_step_vjp_workspace_bytes``: 16 fields and the transform scratch).  The backward passes are first order only: they
are marked ``once_differentiable``, so a double backward raises instead of dropping second-order terms (on an ensemble plan,
``tcfd_fvm_plan_set_ensemble``, already the recorded backward raises ``NotImplementedError``).  Gradients with
respect to the tableau coefficients are not provided (``RKStepper`` raises for a tableau that requires grad).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable


def wants_grad(ux: torch.Tensor, uy: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and (ux.requires_grad or uy.requires_grad)


def cotangent_pair(gx: Optional[torch.Tensor], gy: Optional[torch.Tensor],
                   like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The cotangents of the two output components as contiguous tensors shaped and typed as ``like``; ``None`` (a loss that
    reads one component only) stands for zeros."""
    def one(g):
        if g is None:
            return torch.zeros_like(like, memory_format=torch.contiguous_format)
        return g.to(like.dtype).reshape(like.shape).contiguous()

    return one(gx), one(gy)


def _like(shape, t: torch.Tensor) -> torch.Tensor:
    """A storage-free stand-in of dtype / device of ``t`` and the given shape, for ``cotangent_pair``."""
    return torch.empty((), dtype=t.dtype, device=t.device).expand(shape)


def _refuse_ensemble_double_backward(plan) -> None:
    """A backward that is itself recorded (``create_graph=True``) on an ensemble plan: the adjoint kernels are first order, and
    nothing composed stands behind them for per-sample physics."""
    if torch.is_grad_enabled() and getattr(plan, "members", 0):
        raise NotImplementedError("double backward (create_graph=True) through an ensemble with per-sample viscosity / drag / "
                                  "forcing_scale is not implemented: the adjoint kernels are first order")


class ExplicitTermsFn(torch.autograd.Function):
    """``(kx, ky) = explicit_terms(ux, uy)``; backward: ``J^T (kx_bar, ky_bar)`` by the gather kernel."""

    @staticmethod
    def forward(ctx, plan, dt: float, ux: torch.Tensor, uy: torch.Tensor):
        ctx.set_materialize_grads(False)
        ctx.plan, ctx.dt = plan, dt
        ctx.save_for_backward(ux, uy)
        return plan.explicit_terms(ux, uy, dt)

    @staticmethod
    def backward(ctx, gx, gy):
        _refuse_ensemble_double_backward(ctx.plan)
        return ExplicitTermsFn._backward(ctx, gx, gy)

    @staticmethod
    @once_differentiable
    def _backward(ctx, gx, gy):
        ux, uy = ctx.saved_tensors
        gx, gy = cotangent_pair(gx, gy, ux)
        bx, by = ctx.plan.explicit_terms_vjp(ux, uy, gx, gy, ctx.dt)
        return None, None, bx, by


class ProjectFn(torch.autograd.Function):
    """``P u``; backward: ``P`` of the cotangent (the projection is symmetric)."""

    @staticmethod
    def forward(ctx, plan, ux: torch.Tensor, uy: torch.Tensor):
        ctx.set_materialize_grads(False)
        ctx.plan = plan
        ctx.like = _like(ux.shape, ux)
        return plan.project(ux, uy)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx, gy):
        gx, gy = cotangent_pair(gx, gy, ctx.like)
        return (None, *ctx.plan.project(gx, gy))


class StepFn(torch.autograd.Function):
    """``steps`` RK steps; the forward saves every step's input, the backward runs their reverse in one device call."""

    @staticmethod
    def forward(ctx, plan, dt: float, a: Sequence[float], b: Sequence[float], steps: int, ux: torch.Tensor,
                uy: torch.Tensor):
        ctx.set_materialize_grads(False)
        saved, ox, oy = plan.step_saving(ux, uy, dt, a, b, steps)
        ctx.plan, ctx.dt, ctx.a, ctx.b = plan, dt, tuple(a), tuple(b)
        ctx.save_for_backward(saved)
        return ox, oy

    @staticmethod
    def backward(ctx, gx, gy):
        _refuse_ensemble_double_backward(ctx.plan)
        return StepFn._backward(ctx, gx, gy)

    @staticmethod
    @once_differentiable
    def _backward(ctx, gx, gy):
        (saved,) = ctx.saved_tensors
        gx, gy = cotangent_pair(gx, gy, _like(saved.shape[2:], saved))
        bx, by = ctx.plan.step_vjp(saved, gx, gy, ctx.dt, ctx.a, ctx.b)
        return None, None, None, None, None, bx, by
