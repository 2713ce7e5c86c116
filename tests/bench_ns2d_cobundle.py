#!/usr/bin/env python
"""Cost of K cotangents of one trajectory through the adjoint model: ms per RK4-CN step (forward sweep included) of
  (a) ``adjoint_bundle_step`` on B states with K cotangents each -- one call,
  (b) K calls of ``adjoint_step`` on the B states -- what a user did before; with ``--parent-lib`` on a library built from the
      parent commit, otherwise on this build's,
  (c) ``adjoint_step`` on the state repeated K times in the batch (K B fields with one cotangent each),
  (d) the plain fused step of the B states,
the four alternating inside one process; median and spread (max - min) of five regions timed with device events after a
warm-up (the method of tests/bench_ns2d_bundle.py and tests/bench_ns2d_step_vjp.py).

    python tests/bench_ns2d_cobundle.py [--regions 5] [--steps 20] [--only n,B,K,f64] [--parent-lib path/libtcfd_hip.so] [--variants bundle] [--json out.json]

Pass model (S = B n m 2w bytes: one complex half-spectrum field of the B states; what each launch must read and write once;
RK4-CN is a five-stage schedule).  Per step and per cotangent, ``adjoint_step`` moves 310 S:
    forward sweep 70 S, recomputation of u_1 .. u_4 67 S,
    reversed stages: k_stage_adjoint 23 S, k_cols<MODE_A> 25 S, k_cols<MODE_INV> 10 S, k_rows_vjp 45 S, 4 x k_cols<MODE_FWD> 40 S,
    k_vjp_close 30 S = 173 S.
The bundle moves the state's share once per step -- forward 70 S, recomputation 67 S, MODE_A 25 S, and per cotangent GROUP the
state's four planes in the row pass, 20 S -- and per cotangent 23 + 10 + 25 + 40 + 30 = 128 S:
    bundle  (162 + 20 groups + 128 K) S        K calls  310 K S        ratio at K = 8, one group: 0.486; three groups: 0.502
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
CONFIGS = ((256, 2, 8, "f64"), (1024, 2, 8, "f64"), (1024, 2, 8, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
PLAIN_S, SINGLE_S, STATE_S, GROUP_S, MEMBER_S = 70, 310, 162, 20, 128


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
    """A second build of the library (the parent commit's) with the prototypes of this package's tables."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in {**_lib.SIGNATURES, **_lib.ADJOINT_SIGNATURES}.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.tcfd_version() == _lib.ABI_VERSION, "the parent library has another ABI revision"
    return lib


class using:
    """Everything inside runs on ``lib``: the plans created there keep it."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.old, _lib._lib = _lib.load(), self.lib

    def __exit__(self, *exc):
        _lib._lib = self.old


def groups(op, w0, G):
    """Cotangent groups per chunk of the bundle call, as the library ran them: the row-pass launches of one adjoint sweep of
    the explicit terms on ONE state with the K cotangents, from its per-launch records (``k_rows_vjp_bundle`` is launched once
    per group; the shapes measured here do not run the per-cotangent fall-back).  Where a chunk holds several states every
    cotangent is in one group, so one state gives the count of any chunk."""
    import ns2d_cobundle_ops as CO

    plan = op._plan(w0)
    return CO.row_launches(plan, lambda: plan.explicit_terms_vjp_bundle(w0[:1], G[:, :1].contiguous()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="n,B,K,f64|f32")
    ap.add_argument("--parent-lib", default=None, help="libtcfd_hip.so built from the parent commit: variant (b) runs on it")
    ap.add_argument("--variants", default="bundle,k_calls,replicated,plain", help="which of the four to run (profiling runs: bundle)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns2d_cobundle.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, k_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), int(k_), t_),)
    wanted = args.variants.split(",")
    parent_lib = open_library(args.parent_lib) if args.parent_lib else None
    steps = args.steps
    rows = []
    for n, B, K, tag in configs:
        real = REAL[tag]
        torch.set_default_dtype(real)
        grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
        forcing = tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4)
        make = lambda: tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=forcing, solver=tc.RK4CrankNicolsonStepper()).to(dev)
        op = make()
        dt = tc.stable_time_step(dx=L / n, max_velocity=5.0, max_courant_number=0.5, viscosity=1e-3)
        gen = torch.Generator().manual_seed(n + B)
        k2 = (op.kx**2 + op.ky**2) * L * L
        smooth = torch.exp(-k2 / 64.0)           # smooth fields of moderate amplitude
        w0 = (torch.fft.rfft2(torch.randn(B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev)) * smooth).contiguous()
        G = (torch.fft.rfft2(torch.randn(K, B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev)) * smooth).contiguous()
        w_rep = w0.repeat(K, 1, 1).contiguous()                      # (K B, n, m): copy k of state b is field k B + b
        g_rep = G.reshape(K * B, n, n // 2 + 1)
        single = op
        if parent_lib is not None:
            with using(parent_lib):
                single = make()
                single._plan(w0)                 # the plan is created by, and keeps, the parent library

        def bundle():
            return op.adjoint_bundle_step(w0, G, dt, steps)[1]

        def k_calls():
            return torch.stack([single.adjoint_step(w0, G[k], dt, steps)[1] for k in range(K)])

        def replicated():
            return op.adjoint_step(w_rep, g_rep, dt, steps)[1].reshape(G.shape)

        def plain():
            op(w0, dt, steps)

        variants = [v for v in (("bundle", bundle, 1), ("k_calls", k_calls, 1), ("replicated", replicated, 1), ("plain", plain, 4))
                    if v[0] in wanted]
        outs = {}
        for name, fn, _ in variants:   # warm-up: code objects, workspaces, tables, the allocator's pools
            outs[name] = fn()
            fn()
        torch.cuda.synchronize()
        ref = outs.get("k_calls")
        agree = {} if ref is None else {k: (torch.linalg.norm(v - ref) / torch.linalg.norm(ref)).item()
                                        for k, v in outs.items() if v is not None and k != "k_calls"}
        del outs, ref
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps in variants:
                times[name].append(region(fn, reps) / steps)
        S = B * n * (n // 2 + 1) * 2 * (8 if tag == "f64" else 4)
        ng = groups(op, w0, G)
        model_bundle, model_single = (STATE_S + GROUP_S * ng + MEMBER_S * K) * S, SINGLE_S * K * S
        st = {name: stats(ts) for name, ts in times.items()}
        row = {"n": n, "batch": B, "cotangents": K, "dtype": tag, "steps": steps, "regions": args.regions,
               "cotangent_groups_per_chunk": ng, "k_calls_library": "parent" if parent_lib is not None else "this build",
               "model_bytes_per_step": {"bundle": model_bundle, "k_calls": model_single, "replicated": model_single, "plain": PLAIN_S * S},
               "model_bundle_over_k_calls": model_bundle / model_single, "cotangent_rel_l2_vs_k_calls": agree,
               **{name + "_ms_per_step": v for name, v in st.items()}}
        if "bundle" in st:
            a = st["bundle"]
            gbs = model_bundle / (a["median_ms"] / 1e3) / 1e9
            row.update({"bundle_algorithmic_GBps": gbs, "bundle_fraction_of_8TBps": gbs * 1e9 / PEAK})
            for other in ("k_calls", "replicated"):
                if other in st:
                    b = st[other]
                    row[f"bundle_over_{other}"] = a["median_ms"] / b["median_ms"]
                    # the bar: one bundle call beats the other form by more than the larger of the two spreads
                    row[f"beats_{other}_by_more_than_spread"] = bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"]))
            if "plain" in st:
                row["bundle_over_plain"] = a["median_ms"] / st["plain"]["median_ms"]
                row["expected_over_plain_on_bytes"] = model_bundle / (PLAIN_S * S)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del op, single, w0, G, w_rep, g_rep
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
