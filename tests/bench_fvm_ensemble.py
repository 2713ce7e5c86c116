#!/usr/bin/env python
"""A viscosity / drag sweep on the finite-volume solver as ONE ensemble operator (tcfd_fvm_plan_set_ensemble) against what a
user did before, on one GPU:

    (a) one ensemble call:      NavierStokes2DFVMProjection(viscosity=[...], drag=[...]) on the (B, n, n) state
    (b) a scalar operator on the same batch (one physics for all B fields): the bytes model says (a) / (b) = 1.00 -- the member
        table is 3 B values, read once per workgroup
    (c) B scalar operators, each on its own (1, n, n) field: B plans, B launch-bound calls per step

    python tests/bench_fvm_ensemble.py [--regions 5] [--json profiles/fvm_ensemble_bench.json] [--scalar-ab PARENT_TREE]

The three variants alternate inside every one of `--regions` regions of one process; a region times `steps` calls of a variant
between two device events after a warm-up of every shape.  Reported: the median over the regions and their spread (max - min).
Shapes: 256^2 x 16 fp64, 1024^2 x 16 fp64 and fp32, classic RK4, van Leer; at 1024^2 x 16 fp64 also tangent_step and
forward + backward of one step for (a) against (b).

--scalar-ab PARENT_TREE: the scalar path itself.  PARENT_TREE is a checkout of the parent commit with its library built;
tests/bench_fvm.py runs there and here in alternating fresh processes (`--ab-runs` each), and the 1024^2 x 64 fp64 row of every
run is kept: the two medians and the spread of each side.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = 2 * math.pi
B = 16
SHAPES = ((256, "float64", 200), (1024, "float64", 30), (1024, "float32", 40))     # n, dtype, calls per region
NU = [1e-4 * 100 ** (b / (B - 1)) for b in range(B)]       # 1e-4 .. 1e-2, geometric
DRAG = [0.2 * b / (B - 1) for b in range(B)]                # 0 .. 0.2: member 0 has no drag
NU_MID, DRAG_MID = 1e-3, 0.1                                # the scalar operator of (b)


def summary(times):
    return {"median_ms": statistics.median(times) * 1e3, "spread_ms": (max(times) - min(times)) * 1e3,
            "regions_ms": [t * 1e3 for t in times]}


def measure(variants, calls, regions, warmup=2):
    """variants: name -> a function making ONE call.  Returns name -> per-region seconds per call, the variants alternating
    inside every region."""
    import torch

    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(regions):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            torch.cuda.synchronize()
            out[name].append(t0.elapsed_time(t1) / 1e3 / calls)
    return out


def ensemble_rows(regions):
    import torch

    import torch_cfd_amd as tc
    from torch_cfd_amd import initial_conditions as ic

    dev = torch.device("cuda:0")
    rows = []
    for n, dname, calls in SHAPES:
        dtype = getattr(torch, dname)
        torch.set_default_dtype(dtype)
        grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
        ux, uy = ic.filtered_velocity_field(grid, 3.0, 3.0, random_state=0, device=dev, batch_seeds=list(range(B)))
        forcing = tc.KolmogorovForcing(grid=grid, diam=L, wave_number=3, offsets=grid.cell_faces)
        make = lambda nu, drag: tc.NavierStokes2DFVMProjection(nu, grid, drag=drag, forcing=forcing,
                                                               solver=tc.RKStepper.from_method(method="classic_rk4"))
        dt = tc.stable_time_step(dx=L / n, max_velocity=3.0, max_courant_number=0.5, viscosity=max(NU))
        ens, one, each = make(NU, DRAG), make(NU_MID, DRAG_MID), [make(NU[b], DRAG[b]) for b in range(B)]
        singles = [(ux[b:b + 1].contiguous(), uy[b:b + 1].contiguous()) for b in range(B)]
        with torch.no_grad():
            # the sweep computes the same thing either way: member b of (a) is (c)'s operator b, bit for bit
            got = ens((ux, uy), dt)
            for b in (0, B - 1):
                want = each[b](singles[b], dt)
                assert torch.equal(got[0][b:b + 1], want[0]) and torch.equal(got[1][b:b + 1], want[1]), (n, dname, b)
            t = measure({"a_ensemble": lambda: ens((ux, uy), dt), "b_scalar_same_batch": lambda: one((ux, uy), dt),
                         "c_scalar_per_member": lambda: [each[b](singles[b], dt) for b in range(B)]}, calls, regions)
        row = {"what": "step", "n": n, "batch": B, "dtype": dname, "calls_per_region": calls, "regions": regions}
        row.update({k: summary(v) for k, v in t.items()})
        a, b_, c = (row[k]["median_ms"] for k in ("a_ensemble", "b_scalar_same_batch", "c_scalar_per_member"))
        row["a_over_b"], row["c_over_a"] = a / b_, c / a
        row["a_beats_c_by_more_than_the_spread"] = (c - a) > max(row["a_ensemble"]["spread_ms"], row["c_scalar_per_member"]["spread_ms"])
        row["a_minus_b_within_the_spread"] = abs(a - b_) <= max(row["a_ensemble"]["spread_ms"], row["b_scalar_same_batch"]["spread_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        if n == 1024 and dname == "float64":
            du = (torch.randn_like(ux), torch.randn_like(uy))
            with torch.no_grad():
                t = measure({"a_ensemble": lambda: ens.tangent_step((ux, uy), du, dt),
                             "b_scalar_same_batch": lambda: one.tangent_step((ux, uy), du, dt)}, calls, regions)
            rows.append(pair_row("tangent_step", n, dname, calls, regions, t))

            def fwd_bwd(eq):
                def run():
                    leaves = (ux.clone().requires_grad_(), uy.clone().requires_grad_())
                    out = eq(leaves, dt)
                    ((out[0] * out[0]).sum() + (out[1] * out[1]).sum()).backward()
                return run
            t = measure({"a_ensemble": fwd_bwd(ens), "b_scalar_same_batch": fwd_bwd(one)}, calls, regions)
            rows.append(pair_row("forward_backward", n, dname, calls, regions, t))
        del ens, one, each, singles, ux, uy
        torch.cuda.empty_cache()
    torch.set_default_dtype(torch.float32)
    return rows


def pair_row(what, n, dname, calls, regions, t):
    row = {"what": what, "n": n, "batch": B, "dtype": dname, "calls_per_region": calls, "regions": regions}
    row.update({k: summary(v) for k, v in t.items()})
    a, b_ = row["a_ensemble"]["median_ms"], row["b_scalar_same_batch"]["median_ms"]
    row["a_over_b"] = a / b_
    row["a_minus_b_within_the_spread"] = abs(a - b_) <= max(row["a_ensemble"]["spread_ms"], row["b_scalar_same_batch"]["spread_ms"])
    print(json.dumps(row), flush=True)
    return row


def scalar_ab(parent, runs):
    """tests/bench_fvm.py in the parent's tree and in this one, alternating fresh processes; the 1024^2 x 64 fp64 row of each."""
    got = {"parent": [], "head": []}
    for _ in range(runs):
        for side, root in (("parent", os.path.abspath(parent)), ("head", ROOT)):
            with tempfile.NamedTemporaryFile(suffix=".json") as f:
                subprocess.run([sys.executable, os.path.join(root, "tests", "bench_fvm.py"), "--json", f.name], cwd=root, check=True,
                               stdout=subprocess.DEVNULL, timeout=600)
                rows = json.load(open(f.name))
            row = next(r for r in rows if (r["n"], r["batch"], r["dtype"]) == (1024, 64, "float64"))
            got[side].append(row["ms_per_step"])
            print(json.dumps({"scalar_ab": side, "ms_per_step": row["ms_per_step"]}), flush=True)
    out = {"what": "tests/bench_fvm.py at 1024^2 x 64 fp64, alternating fresh processes", "runs_per_side": runs}
    for side, v in got.items():
        out[side] = {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "runs_ms": v}
    out["medians_within_the_spread"] = (abs(out["parent"]["median_ms"] - out["head"]["median_ms"])
                                        <= max(out["parent"]["spread_ms"], out["head"]["spread_ms"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--scalar-ab", default=None, metavar="PARENT_TREE")
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-ensemble", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    result = json.load(open(args.json)) if args.json and os.path.exists(args.json) else {}     # the two halves may run apart
    if args.scalar_ab:       # first: its child processes then run beside a parent that holds no device memory
        result["scalar_path"] = scalar_ab(args.scalar_ab, args.ab_runs)
    if not args.skip_ensemble:
        result["ensemble"] = ensemble_rows(args.regions)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
