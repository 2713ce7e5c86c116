#!/usr/bin/env python
"""Throughput of the tangent bundle (tcfd_ns2d_step_jvp_bundle, k_rows_jvp_bundle): ms per RK4-CN step of
  (a) ``tangent_bundle_step`` on B states with K tangents each -- one call,
  (b) ``tangent_step`` on the state repeated K times (K B fields with one tangent each) -- what a user did before,
  (c) the plain fused step of the B states,
  (d) (a) on a second operator whose plan was created under TCFD_BUNDLE_ROWS=0: the two-pass row kernels (k_rows_jvp PART 1 once,
      PART 2 per tangent) in place of k_rows_jvp_bundle -- the A/B behind the per-size choice (bundle_two_pass),
the four alternating inside one process; median and spread (max - min) of five regions timed with device events after a
warm-up (the method of tests/bench_ns2d_jvp.py).

    python tests/bench_ns2d_bundle.py [--regions 5] [--steps N] [--only n,B,K,f64] [--variants bundle] [--json out.json]

Pass model (S = B n m 2w bytes: one complex half-spectrum field of the B states).  A stage of the
single-tangent sweep moves 34 S per (state, tangent) pair: 17 S for each of the two.  The bundle moves the state's 17 S once:
    replicated   K x (5 x 34 S - 4 S)         = 166 K S
    bundle       (K + 1) x (5 x 17 S - 2 S)   = 83 (K + 1) S          ratio (K + 1) / (2 K): 0.5625 at K = 8
"""
import argparse
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

PEAK = 8e12
L = 2 * math.pi
CONFIGS = ((256, 2, 8, "f64"), (1024, 2, 8, "f64"), (1024, 2, 8, "f32"))
REAL = {"f64": torch.float64, "f32": torch.float32}
PLAIN_S = 70


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


def two_pass(n, tag):
    """Sizes whose bundle runs the two-pass row kernels instead of k_rows_jvp_bundle.  A COPY of the rule in
    csrc/tcfd_ns2d_sized.hip (bundle_two_pass: max(64, n / ROW_EPT) * 5 * ROW_EPT * sizeof(complex) > 80 KB, ROW_EPT from the Cfg
    rows) -- the library does not export it; it only labels the rows of the record, and must follow that predicate when it moves."""
    return n in (80, 160, 320, 640, 1280, 1536, 2048, 4096) if tag == "f64" else n == 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="steps per library call (0: 20 at 256, 5 at 1024)")
    ap.add_argument("--only", default=None, help="n,B,K,f64|f32")
    ap.add_argument("--variants", default="bundle,replicated,plain,bundle_two_pass", help="which of the four to run (profiling runs: bundle)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns2d_bundle.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    configs = CONFIGS
    if args.only:
        n_, b_, k_, t_ = args.only.split(",")
        configs = ((int(n_), int(b_), int(k_), t_),)
    wanted = args.variants.split(",")
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
        w0 = torch.fft.rfft2(torch.randn(B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev)) * smooth
        dW = torch.fft.rfft2(torch.randn(K, B, n, n, generator=gen, dtype=torch.float64).to(real).to(dev)) * smooth * 1e-3
        w_rep = w0.repeat(K, 1, 1).contiguous()                      # (K B, n, m): copy k of state b is field k B + b
        dw_rep = dW.reshape(K * B, n, n // 2 + 1)
        steps = args.steps or (20 if n <= 256 else 5)

        def bundle():
            op.tangent_bundle_step(w0, dW, dt, steps)

        def replicated():
            op.tangent_step(w_rep, dw_rep, dt, steps)

        def plain():
            op(w0, dt, steps)

        op2 = None
        if "bundle_two_pass" in wanted and not two_pass(n, tag):
            os.environ["TCFD_BUNDLE_ROWS"] = "0"          # read once, when the plan is created
            try:
                op2 = make()
                op2.tangent_bundle_step(w0, dW, dt, 1)
            finally:
                del os.environ["TCFD_BUNDLE_ROWS"]

        def bundle_two_pass():
            op2.tangent_bundle_step(w0, dW, dt, steps)

        variants = [v for v in (("bundle", bundle, 2), ("replicated", replicated, 2), ("plain", plain, 4),
                                ("bundle_two_pass", bundle_two_pass, 2)) if v[0] in wanted and (v[0] != "bundle_two_pass" or op2 is not None)]
        for _, fn, _ in variants:   # warm-up: code objects, workspaces
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, *_ in variants}
        for _ in range(args.regions):
            for name, fn, reps in variants:
                times[name].append(region(fn, reps) / steps)
        S = B * n * (n // 2 + 1) * 2 * (8 if tag == "f64" else 4)
        model_bundle, model_rep = 83 * (K + 1) * S, 166 * K * S
        row = {"n": n, "batch": B, "tangents": K, "dtype": tag, "steps_per_call": steps, "regions": args.regions,
               "row_pass": "two-pass fall-back (k_rows_jvp PART 1 + K x PART 2)" if two_pass(n, tag) else "k_rows_jvp_bundle",
               "model_bytes_per_step": {"bundle": model_bundle, "replicated": model_rep, "plain": PLAIN_S * S},
               "model_bundle_over_replicated": (K + 1) / (2 * K)}
        st = {name: stats(ts) for name, ts in times.items()}
        for name, s in st.items():
            row[name + "_ms"] = s
        if "bundle" in st:
            a = st["bundle"]
            gbs = model_bundle / (a["median_ms"] / 1e3) / 1e9
            row["bundle_algorithmic_GBps"] = gbs
            row["bundle_fraction_of_8TBps"] = gbs * 1e9 / PEAK
            if "replicated" in st:
                b = st["replicated"]
                row["bundle_over_replicated"] = a["median_ms"] / b["median_ms"]
                # the bar: one bundle call beats the replicated call by more than the larger of the two spreads
                row["beats_replicated_by_more_than_spread"] = bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"]))
            if "bundle_two_pass" in st:
                row["bundle_over_two_pass_rows"] = a["median_ms"] / st["bundle_two_pass"]["median_ms"]
            if "plain" in st:
                row["bundle_over_plain"] = a["median_ms"] / st["plain"]["median_ms"]
                row["expected_over_plain_on_bytes"] = model_bundle / (PLAIN_S * S)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del op, w0, dW, w_rep, dw_rep
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
