#!/usr/bin/env python
"""Cost of a gradient through the fused spectral step: ms per RK4-CN step of forward + backward through ``op.forward`` with a
state that requires grad, on the one-node path (``FusedSteps``: fused forward step per step + one tcfd_ns2d_step_vjp call), on
the per-stage node chain of the same build (``TCFD_FUSED_ADJOINT=0``) and -- with ``--parent-lib`` -- on the per-stage chain
running a library built from the parent commit, next to the forward-only fused step; all alternating inside one process,
median and spread (max - min) of five regions timed with device events after a warm-up.

    python tests/bench_ns2d_step_vjp.py [--regions 5] [--steps 20] [--only n,B,f64] [--parent-lib path/libtcfd_hip.so] [--json out.json]

Pass model (S = B n m 2w bytes, one complex half-spectrum field; what each launch must read and write once), per RK4-CN step:
    forward             the fused step, its result written into the next saved slot            70 S   
    recomputation       stages 0 .. 3: k_cols<MODE_A> 5 S, row pass 5 S, k_cols<MODE_F> 2 S,
                        k_stage_update 5 S (4 S at the first stage)                            4 x 17 S - 1 S = 67 S
    reversed stage      k_stage_adjoint 5 S (4 S at the first and the last stage), k_cols<MODE_A> 5 S, k_cols<MODE_INV> 2 S,
                        k_rows_vjp 9 S, 4 x k_cols<MODE_FWD> 8 S, k_vjp_close 6 S              5 x 35 S - 2 S = 173 S
    forward + backward  310 S = 4.4 x the forward step
The per-stage chain runs ONE forward sweep (85 S) and keeps the stage states; the one-node path runs two (70 S + 67 S) and keeps
one field per step.  Its reversal is cheaper (one launch where the chain has one plus a dozen tensor-op launches), the second
sweep is not paid back: DESIGN section 20 has the measured split per kernel.  ``--variants`` runs one path per process, for
kernel traces.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd import _lib  # noqa: E402

PEAK = 8e12
L = 2 * math.pi
CONFIGS = ((256, 16, "f64"), (1024, 16, "f64"), (1024, 16, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
FORWARD_S, MODEL_S = 70, 310


def region(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / reps


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "spread_ms": (max(ts) - min(ts)) * 1e3}


def open_library(path):
    """A second build of the library (the parent commit's) with the prototypes of this package's table."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.tcfd_version() == _lib.ABI_VERSION, "the parent library has another ABI revision"
    return lib


class using:
    """Everything inside runs on ``lib``: the plans created there keep it, and the per-stage nodes look the global one up."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.old, _lib._lib = _lib.load(), self.lib

    def __exit__(self, *exc):
        _lib._lib = self.old


def make_op(n, dev):
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
    return tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="n,B,f64|f32")
    ap.add_argument("--parent-lib", default=None, help="libtcfd_hip.so built from the parent commit (A/B in one process)")
    ap.add_argument("--variants", default=None, help="comma list of fused_adjoint, per_stage_nodes, parent_library, forward_only "
                    "(profiling runs: one path per process)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns2d_step_vjp.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), t_),)
    this_lib = _lib.load()
    parent_lib = open_library(args.parent_lib) if args.parent_lib else None
    K = args.steps
    rows = []
    for n, B, tag in configs:
        real = REAL[tag]
        torch.set_default_dtype(real)
        op = make_op(n, dev)
        dt = tc.stable_time_step(dx=L / n, max_velocity=5.0, max_courant_number=0.5, viscosity=1e-3)
        gen = torch.Generator().manual_seed(n + B)
        w0 = torch.fft.rfft2(torch.randn(B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev))
        k2 = (op.kx**2 + op.ky**2) * L * L
        w0 = (w0 * torch.exp(-k2 / 64.0)).contiguous()          # a smooth state of moderate amplitude
        cot = torch.view_as_real(torch.roll(w0, 1, 0)).contiguous()
        ops = {"this": op}
        if parent_lib is not None:
            with using(parent_lib):
                ops["parent"] = make_op(n, dev)
                ops["parent"]._plan(w0)             # the plan is created by, and keeps, the parent library

        def grad_step(which, flag, lib):
            def run():
                os.environ["TCFD_FUSED_ADJOINT"] = flag
                with using(lib):
                    w = w0.detach().requires_grad_(True)
                    out, _ = ops[which](w, dt, K)
                    (torch.view_as_real(out) * cot).sum().backward()
                    return w.grad
            return run

        def forward_only():
            op(w0, dt, K)

        variants = [("fused_adjoint", grad_step("this", "1", this_lib), 1), ("per_stage_nodes", grad_step("this", "0", this_lib), 1)]
        if parent_lib is not None:
            variants.append(("parent_library", grad_step("parent", "0", parent_lib), 1))
        variants.append(("forward_only", forward_only, 2))
        if args.variants:
            variants = [v for v in variants if v[0] in args.variants.split(",")]
        grads = {}
        for name, fn, _ in variants:   # warm-up: code objects, workspaces, tables, the allocator's pools
            grads[name] = fn()
            fn()
        torch.cuda.synchronize()
        ref = grads.get("per_stage_nodes")
        agree = {} if ref is None else {k: (torch.linalg.norm(v - ref) / torch.linalg.norm(ref)).item()
                                        for k, v in grads.items() if v is not None}
        del grads, ref
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps in variants:
                times[name].append(region(fn, reps) / K)
        os.environ.pop("TCFD_FUSED_ADJOINT", None)
        S = B * n * (n // 2 + 1) * 2 * (8 if tag == "f64" else 4)
        st = {name: stats(ts) for name, ts in times.items()}
        row = {"n": n, "batch": B, "dtype": tag, "steps": K, "regions": args.regions,
               **{name + "_ms_per_step": v for name, v in st.items()}, "gradient_rel_l2_vs_per_stage_nodes": agree}
        base_name = "parent_library" if "parent_library" in st else "per_stage_nodes"
        if "fused_adjoint" in st:
            new = st["fused_adjoint"]
            gbs = MODEL_S * S / (new["median_ms"] / 1e3) / 1e9
            row.update({"expected_on_bytes": MODEL_S / FORWARD_S, "model_bytes_per_step": MODEL_S * S, "algorithmic_GBps": gbs,
                        "fraction_of_8TBps": gbs * 1e9 / PEAK})
            if "forward_only" in st:
                row["over_forward_step"] = new["median_ms"] / st["forward_only"]["median_ms"]
            if base_name in st:
                base = st[base_name]
                # the bar: faster than the parent's path by more than the larger spread of the two
                row.update({"baseline": base_name, "speedup_vs_baseline": base["median_ms"] / new["median_ms"],
                            "beats_baseline_by_more_than_spread": bool(
                                base["median_ms"] - new["median_ms"] > max(base["spread_ms"], new["spread_ms"]))})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del op, ops, w0, cot
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
