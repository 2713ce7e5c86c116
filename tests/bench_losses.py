#!/usr/bin/env python
"""Timing of ResidualLoss and LpLoss (csrc/tcfd_residual.hip) next to the plain-torch restatement tests/losses_ops.py on the same
GPU, in the same process, alternating call by call.

    python tests/bench_losses.py [--json profiles/losses_bench.json]

Per shape: device events around one call (forward, and forward + backward with respect to w and f), after a warm-up, median of
five.  Algorithmic bytes follow the pass model of DESIGN (A = b n^2 T w bytes of one real tensor): the fused forward moves 34 A,
forward + backward 112 A; the fraction of 8 TB/s is reported on that model.  LpLoss: x and y read once forward (2 A), read again
and the gradient written backward (3 A)."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import losses_ops as ops  # noqa: E402
from torch_cfd_amd.losses import LpLoss, ResidualLoss  # noqa: E402

PEAK = 8e12
RESIDUAL_SHAPES = ((32, 256, 10, torch.float32), (4, 64, 40, torch.float64), (8, 256, 10, torch.float64))
RES_FWD_A, RES_FWD_BWD_A = 34, 112


def alternating_ms(fn_a, fn_b, warmup=2, repeats=5):
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            acc.append(t0.elapsed_time(t1))
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for b, n, nt, dtype in RESIDUAL_SHAPES:
        torch.set_default_dtype(dtype)
        g = torch.Generator(device=dev).manual_seed(0)
        w = (40 * torch.randn(b, n, n, nt, device=dev, generator=g)).requires_grad_(True)
        f = (300 * torch.randn(b, n, n, nt, device=dev, generator=g)).requires_grad_(True)
        visc, dt = ops.residual_visc(n), ops.RESIDUAL_DELTA_T
        m = ResidualLoss(batch_size=b, visc=visc, n_grid=n, n_t=nt, delta_t=dt)
        ref = lambda: ops.residual_loss(w, f=f, visc=visc, delta_t=dt)

        def hip_fwd():
            with torch.no_grad():
                return m(w, f=f)

        def ops_fwd():
            with torch.no_grad():
                return ref()

        def hip_both():
            return torch.autograd.grad(m(w, f=f), (w, f))

        def ops_both():
            return torch.autograd.grad(ref(), (w, f))

        err = abs(float(hip_fwd()) - float(ops_fwd())) / abs(float(ops_fwd()))
        gh, go = hip_both(), ops_both()
        gerr = float(torch.linalg.norm(gh[0] - go[0]) / torch.linalg.norm(go[0]))
        del gh, go
        A = b * n * n * nt * w.element_size()
        row = {"loss": "ResidualLoss", "shape": [b, n, n, nt], "dtype": str(dtype).replace("torch.", ""), "A_bytes": A,
               "rel_err_value_vs_ops": err, "rel_l2_grad_w_vs_ops": gerr}
        for tag, hip, op, units in (("forward", hip_fwd, ops_fwd, RES_FWD_A), ("forward_backward", hip_both, ops_both, RES_FWD_BWD_A)):
            t_hip, t_ops = alternating_ms(hip, op)
            row[tag] = {"hip_ms": t_hip, "torch_ops_ms": t_ops, "speedup_vs_torch_ops": t_ops / t_hip, "algorithmic_bytes": units * A,
                        "fraction_of_8TBps": units * A / (t_hip * 1e-3) / PEAK}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del w, f, m
        torch.cuda.empty_cache()
    # relative L2 of the FNO baselines at the SFNO output block
    torch.set_default_dtype(torch.float32)
    b, n, nt = 32, 256, 10
    x = torch.randn(b, n, n, nt, device=dev).requires_grad_(True)
    y = torch.randn(b, n, n, nt, device=dev)
    lp = LpLoss(p=2, relative=True)
    hip = lambda: torch.autograd.grad(lp(x, y), x)
    op = lambda: torch.autograd.grad(ops.lp_loss(x, y, p=2, relative=True), x)
    err = float(torch.linalg.norm(hip()[0] - op()[0]) / torch.linalg.norm(op()[0]))
    t_hip, t_ops = alternating_ms(hip, op)
    A = x.numel() * 4
    row = {"loss": "LpLoss relative p=2", "shape": [b, n, n, nt], "dtype": "float32", "A_bytes": A, "rel_l2_grad_vs_ops": err,
           "forward_backward": {"hip_ms": t_hip, "torch_ops_ms": t_ops, "speedup_vs_torch_ops": t_ops / t_hip, "algorithmic_bytes": 5 * A,
                                "fraction_of_8TBps": 5 * A / (t_hip * 1e-3) / PEAK}}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
