#!/usr/bin/env python
"""Throughput of the finite-volume step per advection scheme (the SCHEME instantiations of k_fvm_stage / k_fvm_stage_vjp in
tcfd_fvm.hip): steps/s of classic RK4 at 256^2 x 1 and 1024^2 x 16 fp64, forward + backward at 256^2 x 1 fp64, each next
to the plain-torch restatement tests/fvm_schemes_ops.py on the same GPU, and the stage kernels' share of the kernel time.

    python tests/bench_fvm_schemes.py [--steps K] [--warmup W] [--json profiles/fvm_schemes_bench.json] [--no-profile]

The kernel shares come from one `rocprofv3 --kernel-trace --stats` run of a fresh child process (this script with
--trace-child: the same number of 1024^2 x 16 steps and of 256^2 forward + backward rollouts per scheme, no torch-ops
baseline, no counters).  Every other kernel (projection, RK bookkeeping, copies) is launched the same number of times for
every scheme, so a quarter of their total is taken as one scheme's part; a scheme's kernel time is then its k_fvm_stage
time (forward steps and the stages the backward recomputes) + its k_fvm_stage_vjp time + that quarter, and the two shares
reported are k_fvm_stage and k_fvm_stage_vjp over that sum."""
import argparse
import csv
import glob
import json
import math
import os
import re
import subprocess
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import fvm_schemes_ops as S  # noqa: E402
import torch_cfd_amd as tc  # noqa: E402
from torch_cfd_amd import initial_conditions as ic  # noqa: E402

L = 2 * math.pi
SCHEMES = ("van_leer", "upwind", "linear", "lax_wendroff")
SCHEME_ID = {"van_leer": 0, "upwind": 1, "linear": 2, "lax_wendroff": 3}   # the template argument in the kernel names
FORWARD = ((256, 1), (1024, 16))
GRAD = (256, 1)
TRACE_STEPS, TRACE_ROLLOUTS, GRAD_K = 20, 3, 20


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / reps


def dot(u, cot):
    return (u[0] * cot[:, 0]).sum() + (u[1] * cot[:, 1]).sum()


def setup(scheme, n, B, dev):
    """The configuration of tests/bench_fvm.py (nu = 1e-3, drag 0.1, Kolmogorov k = 3, max velocity 3) with `scheme`."""
    ph = S.Physics(scheme, n, nu=1e-3, drag=0.1, wave=3)
    eq = ph.equation(tc.RKStepper.from_method(method="classic_rk4"))
    ux, uy = ic.filtered_velocity_field(ph.grid(), 3.0, 3.0, random_state=0, device=dev, batch_seeds=list(range(B)))
    dt = tc.stable_time_step(dx=L / n, max_velocity=3.0, max_courant_number=0.5, viscosity=1e-3)
    return ph, eq, (ux.detach(), uy.detach()), dt


def measure(args, dev):
    rows = []
    for scheme in SCHEMES:
        row = {"scheme": scheme, "dtype": "float64"}
        for n, B in FORWARD:
            ph, eq, u0, dt = setup(scheme, n, B, dev)
            a, b = eq.solver.weights(dt)
            state, ref = [u0], [u0]
            run = ph.rollout(a, b, dt, 1, dev)
            with torch.no_grad():
                def hip():
                    state[0] = eq(state[0], dt, steps=1)

                def ops():
                    ref[0] = run(ref[0])
                t_hip = timed(hip, args.steps, args.warmup)
                t_ops = timed(ops, args.torch_steps, 1)
            tag = f"{n}x{B}"
            row[f"steps_per_s_{tag}"] = 1 / t_hip
            row[f"torch_ops_steps_per_s_{tag}"] = 1 / t_ops
            row[f"speedup_vs_torch_ops_{tag}"] = t_ops / t_hip
            del state, ref, eq
            torch.cuda.empty_cache()
        n, B = GRAD
        ph, eq, u0, dt = setup(scheme, n, B, dev)
        a, b = eq.solver.weights(dt)
        cot = torch.randn(B, 2, n, n, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
        run = ph.rollout(a, b, dt, 1, dev)

        def hip_grad():
            u = (u0[0].clone().requires_grad_(), u0[1].clone().requires_grad_())
            torch.autograd.grad(dot(eq(u, dt, steps=GRAD_K), cot), u)

        def ops_grad():
            u = (u0[0].clone().requires_grad_(), u0[1].clone().requires_grad_())
            torch.autograd.grad(dot(run(u), cot), u)
        t_hip = timed(hip_grad, 3, 1) / GRAD_K
        t_ops = timed(ops_grad, 2, 1)
        tag = f"{n}x{B}"
        row[f"fwd_bwd_steps_per_s_{tag}"] = 1 / t_hip
        row[f"torch_ops_fwd_bwd_steps_per_s_{tag}"] = 1 / t_ops
        row[f"fwd_bwd_speedup_vs_torch_ops_{tag}"] = t_ops / t_hip
        rows.append(row)
        print(json.dumps(row), flush=True)
        del eq
        torch.cuda.empty_cache()
    base = rows[0]
    for row in rows:
        row["steps_per_s_1024x16_over_van_leer"] = row["steps_per_s_1024x16"] / base["steps_per_s_1024x16"]
    return rows


def trace_child(dev):
    """The work the profiler sees: per scheme, the same steps and rollouts."""
    for scheme in SCHEMES:
        _, eq, u0, dt = setup(scheme, 1024, 16, dev)
        with torch.no_grad():
            u = u0
            for _ in range(TRACE_STEPS):
                u = eq(u, dt)
        del eq, u
        n, B = GRAD
        _, eq, u0, dt = setup(scheme, n, B, dev)
        cot = torch.randn(B, 2, n, n, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
        for _ in range(TRACE_ROLLOUTS):
            u = (u0[0].clone().requires_grad_(), u0[1].clone().requires_grad_())
            torch.autograd.grad(dot(eq(u, dt, steps=GRAD_K), cot), u)
        torch.cuda.synchronize()
        del eq
        torch.cuda.empty_cache()


def profile(out_dir):
    """One rocprofv3 kernel trace of a fresh child; returns ({kernel name: total ns}, path of the stats file)."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--",
           sys.executable, os.path.abspath(__file__), "--trace-child"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 failed:\n" + r.stdout.decode(errors="replace")[-4000:])
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one kernel_stats.csv under {out_dir}, found {files}")
    totals = {}
    with open(files[0]) as f:
        for rec in csv.DictReader(f):
            totals[rec["Name"]] = totals.get(rec["Name"], 0) + int(float(rec["TotalDurationNs"]))
    return totals, files[0]


def shares(totals):
    """Per scheme: kernel time of its fp64 stage kernel and of its stage adjoint, and the share of each in the scheme's
    kernel time.  The child runs the same launches for every scheme apart from these two kernels, so the rest is split
    evenly."""
    def of(prefix, sid):
        pat = re.compile(r"\b" + prefix + r"<\s*" + str(sid) + r"\s*,\s*double\s*>")
        return sum(t for name, t in totals.items() if pat.search(name))

    stage_all = sum(t for name, t in totals.items() if "k_fvm_stage" in name)
    other = (sum(totals.values()) - stage_all) / len(SCHEMES)
    out = {}
    for scheme, sid in SCHEME_ID.items():
        fwd, adj = of("k_fvm_stage", sid), of("k_fvm_stage_vjp", sid)
        if not fwd or not adj:
            raise RuntimeError(f"no k_fvm_stage / k_fvm_stage_vjp kernel of scheme {sid} in the trace: {sorted(totals)}")
        total = fwd + adj + other
        out[scheme] = {"stage_kernel_ms": fwd / 1e6, "stage_vjp_kernel_ms": adj / 1e6, "other_kernels_ms": other / 1e6,
                       "stage_share_of_kernel_time": fwd / total, "stage_vjp_share_of_kernel_time": adj / total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "fvm_schemes_bench.json"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--keep-stats", default=None, help="copy the profiler's kernel_stats.csv here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fvm_schemes.py needs a HIP device")
    dev = torch.device("cuda:0")
    torch.set_default_dtype(torch.float64)
    if args.trace_child:
        trace_child(dev)
        return
    result = {"rows": measure(args, dev)}
    with open(args.json, "w") as f:   # the rates are on disk before the profiler starts
        json.dump(result, f, indent=1)
    if not args.no_profile:
        with tempfile.TemporaryDirectory() as tmp:
            totals, stats = profile(tmp)
            if args.keep_stats:   # only the kernels this script is about, and the largest of the others
                with open(stats) as src:
                    lines = src.read().splitlines()
                keep = [lines[0]] + [ln for k, ln in enumerate(lines[1:]) if "k_fvm_" in ln or k < 12]
                with open(args.keep_stats, "w") as dst:
                    dst.write("\n".join(keep) + "\n")
        result["kernel_shares"] = shares(totals)
        print(json.dumps(result["kernel_shares"]), flush=True)
    rows = result["rows"]
    result["bars"] = {
        "every_scheme_faster_than_its_restatement": all(
            r[k] > 1 for r in rows for k in ("speedup_vs_torch_ops_256x1", "speedup_vs_torch_ops_1024x16",
                                              "fwd_bwd_speedup_vs_torch_ops_256x1")),
        "no_new_scheme_slower_than_van_leer_at_1024x16": all(r["steps_per_s_1024x16_over_van_leer"] >= 1 for r in rows[1:]),
    }
    print(json.dumps(result["bars"]), flush=True)
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
