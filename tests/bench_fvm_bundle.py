#!/usr/bin/env python
"""Throughput of the finite-volume tangent bundle (k_fvm_stage_jvp_bundle on a bundle plan, tcfd_fvm_plan_set_tangent_bundle):
ms per classic-RK4 step, van Leer advection, of
  (a) ``tangent_bundle_step`` on B states with K tangents each -- one call,
  (b) ``tangent_step`` on the state repeated K times (K B pairs) -- what a user did before; with ``--parent-lib`` on a library
      built from the parent commit,
  (c) the plain step of the B states,
the three alternating inside one process; median and spread (max - min) of five regions timed with device events after a
warm-up (the method of tests/bench_fvm_jvp.py).  The bar: (a) is faster than (b) by more than the larger of the two spreads at
1024^2 x 2 in both precisions; 256^2 is launch-bound and reported only.

    python tests/bench_fvm_bundle.py [--regions 5] [--steps N] [--only n,B,K,f64] [--parent-lib path/libtcfd_hip.so] [--json out.json]
    python tests/bench_fvm_bundle.py --jvp-ab path/libtcfd_hip.so [--rounds 3] [--json out.json]

The second form shows that ``tangent_step`` itself has not moved: tests/bench_fvm_jvp.py (--no-torch) on the parent's library and
on this build, in alternating fresh processes; the record holds both medians and spreads per round.

Bytes model, from the launch list of tcfd_fvm_step (F = B n^2 w bytes: one real field of the B states; a call carries N such
fields per array: N = 1 + K for the bundle, 2 K for the replicated pairs, 1 for the plain step).  Every pass is per field:
    k_fvm_div        reads ux, uy, writes div                              3 F
    rfft2            reads div, writes the half spectrum (~ one field)     2 F
    k_fvm_mul        reads and writes the spectrum                         2 F
    irfft2           reads the spectrum, writes q                          2 F   (its internal scratch passes not counted)
    k_fvm_apply      reads P_x, P_y, q, writes u_x, u_y                    5 F
                                                            projection:   14 F per stage, 56 F per step
    stage kernel     reads u_x, u_y once (the stencil's neighbours come from cache), per target reads u0 or the target and
                     writes the target, both components.  Classic RK4: stage 0 writes the next stage state and the final sum
                     from u0 = u (6 F), stages 1 and 2 the next stage state from u0 and add to the final sum (10 F each),
                     stage 3 adds to the final sum (6 F)                  32 F per step
    total            88 N F per step (the forcing table, one (n, n) plane per component read by the state fields alone, and the
                     two copies per CALL left out)
so bundle / replicated = (1 + K) / (2 K) on bytes: 0.5625 at K = 8.  The model is reported beside the measured ratio, not
asserted: the stage kernel is arithmetic-heavy (the van Leer tangent), and 256^2 is bound by its 24 launches per step.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fvm_schemes_ops as S  # noqa: E402
import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd import _lib  # noqa: E402
from torch_cfd_amd import initial_conditions as ic  # noqa: E402

PEAK = 8e12
CONFIGS = ((256, 2, 8, "f64"), (1024, 2, 8, "f64"), (1024, 2, 8, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
MODEL_F = 88   # fields moved per step and per field carried (the docstring's launch list)


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
    for name, (res, args) in _lib.SIGNATURES.items():
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


def jvp_child(lib_path, out):
    """One fresh process of tests/bench_fvm_jvp.py on the library at ``lib_path`` (None: this build's)."""
    code = ("import sys, runpy; sys.path.insert(0, %r); sys.path.insert(0, %r); import torch_cfd_amd._lib as l\n"
            "if %r: l.LIB_PATH = %r\n"
            "sys.argv = ['bench_fvm_jvp.py', '--no-torch', '--json', %r]; runpy.run_path(%r, run_name='__main__')"
            % (os.path.dirname(HERE), HERE, bool(lib_path), os.path.abspath(lib_path) if lib_path else "", out,
               os.path.join(HERE, "bench_fvm_jvp.py")))
    subprocess.run([sys.executable, "-c", code], check=True, stdout=subprocess.DEVNULL)
    with open(out) as f:
        return json.load(f)


def jvp_ab(parent, rounds):
    """bench_fvm_jvp.py on the parent's library and on this build, alternating, a fresh process each."""
    record = []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for which, path in (("parent", parent), ("head", None)):
                for row in jvp_child(path, os.path.join(tmp, "jvp.json")):
                    rec = {"round": r, "library": which, "n": row["n"], "batch": row["batch"], "dtype": row["dtype"],
                           "tangent_step_ms": row["tangent_step_ms"], "plain_step_ms": row["plain_step_ms"]}
                    record.append(rec)
                    print(json.dumps(rec), flush=True)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="steps per library call (0: 20 at 256, 5 at 1024)")
    ap.add_argument("--only", default=None, help="n,B,K,f64|f32")
    ap.add_argument("--parent-lib", default=None, help="libtcfd_hip.so built from the parent commit: variant (b) runs on it")
    ap.add_argument("--jvp-ab", default=None, metavar="PARENT_LIB", help="run tests/bench_fvm_jvp.py on that library and on this "
                    "build in alternating fresh processes, and nothing else")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of --jvp-ab")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.jvp_ab:   # before this process touches the device: the children measure alone
        record = jvp_ab(args.jvp_ab, args.rounds)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(record, f, indent=1)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_fvm_bundle.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, k_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), int(k_), t_),)
    parent_lib = open_library(args.parent_lib) if args.parent_lib else None
    rows = []
    for n, B, K, tag in configs:
        real = REAL[tag]
        torch.set_default_dtype(torch.float64)
        ph = S.Physics("van_leer", n, wave=4)
        make = lambda: ph.equation(tc.RKStepper.from_method(method="classic_rk4"))
        eq = make()
        dt = tc.stable_time_step(dx=ph.h, max_velocity=2.0, max_courant_number=0.5, viscosity=ph.nu)
        u = tuple(c.detach().to(real).contiguous() for c in
                  ic.filtered_velocity_field(ph.grid(), 2.0, 3.0, random_state=0, device=dev, batch_seeds=list(range(B))))
        dV = tuple(torch.stack([1e-3 * torch.roll(c, (1 + k, 3 + 2 * k), (-2, -1)) for k in range(K)]).contiguous() for c in u)
        u_rep = tuple(c.repeat(K, 1, 1).contiguous() for c in u)             # (K B, n, n): copy k of state b is field k B + b
        dv_rep = tuple(c.reshape(K * B, n, n) for c in dV)
        steps = args.steps or (20 if n <= 256 else 5)
        single = make()
        if parent_lib is not None:
            with using(parent_lib):
                single._plan(real, dev, tangent=True)       # the plan is created by, and keeps, the parent library

        def bundle():
            eq.tangent_bundle_step(u, dV, dt, steps)

        def replicated():
            single.tangent_step(u_rep, dv_rep, dt, steps)

        def plain():
            eq(u, dt, steps)

        variants = (("bundle", bundle, 2), ("replicated", replicated, 2), ("plain", plain, 4))
        # the three compute the same thing: member k of the bundle has the bits of pair k B + b of the replicated call
        out_a, out_b = eq.tangent_bundle_step(u, dV, dt, steps), single.tangent_step(u_rep, dv_rep, dt, steps)
        same = all(torch.equal(a.reshape(K * B, n, n), b) for a, b in zip(out_a[1], out_b[1]))
        for _, fn, _ in variants:   # warm-up: code objects, workspaces
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps in variants:
                times[name].append(region(fn, reps) / steps)
        F = B * n * n * (8 if tag == "f64" else 4)
        st = {name: stats(ts) for name, ts in times.items()}
        a, b = st["bundle"], st["replicated"]
        gbs = MODEL_F * (1 + K) * F / (a["median_ms"] / 1e3) / 1e9
        row = {"n": n, "batch": B, "tangents": K, "dtype": tag, "scheme": "van_leer", "method": "classic_rk4",
               "steps_per_call": steps, "regions": args.regions,
               "replicated_library": "parent" if parent_lib is not None else "this build",
               "bundle_members_bit_equal_to_replicated": bool(same),
               "bundle_ms": a, "replicated_ms": b, "plain_ms": st["plain"],
               "bundle_over_replicated": a["median_ms"] / b["median_ms"],
               "model_bundle_over_replicated": (1 + K) / (2 * K),
               "model_bytes_per_step": {"bundle": MODEL_F * (1 + K) * F, "replicated": MODEL_F * 2 * K * F, "plain": MODEL_F * F},
               "bundle_over_plain": a["median_ms"] / st["plain"]["median_ms"], "expected_over_plain_on_bytes": 1 + K,
               "bundle_algorithmic_GBps": gbs, "bundle_fraction_of_8TBps": gbs * 1e9 / PEAK,
               # the bar: one bundle call beats the replicated call by more than the larger of the two spreads
               "beats_replicated_by_more_than_spread": bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"])),
               "bar_applies": n >= 1024}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del eq, single, u, dV, u_rep, dv_rep, out_a, out_b
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
