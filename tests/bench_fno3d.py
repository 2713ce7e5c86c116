#!/usr/bin/env python
"""FNO3d baseline: training iteration and forward, timed three ways in ONE process.

  hip        torch_cfd_amd.fno.FNO3d (rectangular lifting kernel, one autograd node per Fourier layer, folded / fused head)
  torch_ops  tests/fno3d_ops.py: rfftn / einsum / irfftn and channel einsums on the same parameters (torch autograd)
  composed   what could be assembled before FNO3d existed: SpectralConv3d with torch modules around it (TCFD_FNO3D_FUSED=0)

Rows: (i) the notebook's iteration -- FNO3d(32, 32, 5, 10, input_channel=10), batch 4, 64 x 64 x 10, relative L2 SobolevLoss, Adam;
(ii) a bandwidth-sized one -- FNO3d(24, 24, 5, 20) at (32, 13, 256, 256, 10).  The three variants alternate window by window;
every window is device-synchronised at both ends; the figure of a variant is the MEDIAN of its windows.  The composed variant
of row (ii) gets single-iteration windows and a time limit of its own (torch's 1x1x1 Conv3d backward is very slow on ROCm at this
size): when it runs out, what it managed is reported with "finished": false.  Peak memory: max_memory_allocated over one
training iteration of a variant, measured in a round of its own.

Row 3 (--rows 3) times the GELU head alone at 2^22 points (it is not part of the default model of rows 1 / 2).

    python tests/bench_fno3d.py [--rows 1,2] [--windows 5] [--out profiles/fno3d_bench.json] [--only hip] [--iters N]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fno3d_ops as ops  # noqa: E402
from torch_cfd_amd import fno  # noqa: E402

ROWS = {
    1: dict(name="notebook", args=(32, 32, 5, 10), kw={"input_channel": 10}, shape=(4, 13, 64, 64, 10), iters=20, warmup=5,
            composed_iters=20, composed_limit_s=120.0),
    2: dict(name="bandwidth", args=(24, 24, 5, 20), kw={}, shape=(32, 13, 256, 256, 10), iters=3, warmup=2,
            composed_iters=1, composed_limit_s=150.0),
}


def make_variants(row, dev):
    torch.manual_seed(0)
    model = fno.FNO3d(*row["args"], **row["kw"]).to(dev)
    n = row["shape"][2]
    loss_fn = fno.SobolevLoss(n_grid=n, norm_order=0, relative=True, time_average=True).to(dev)
    x = torch.randn(*row["shape"], device=dev)
    y = torch.randn(row["shape"][0], *row["shape"][2:], device=dev)
    variants = {}

    def module_variant(m, fused):
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)

        def train():
            os.environ["TCFD_FNO3D_FUSED"] = "1" if fused else "0"
            opt.zero_grad(set_to_none=True)
            out, _ = m(x)
            loss_fn(out, y).backward()
            opt.step()

        def forward():
            os.environ["TCFD_FNO3D_FUSED"] = "1" if fused else "0"
            with torch.no_grad():
                m(x)
        return train, forward

    variants["hip"] = module_variant(model, True)
    twin = fno.FNO3d(*row["args"], **row["kw"]).to(dev)
    twin.load_state_dict(model.state_dict())
    variants["composed"] = module_variant(twin, False)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt_ops = torch.optim.Adam(list(sd.values()), lr=1e-3)

    def ops_train():
        opt_ops.zero_grad(set_to_none=True)
        loss_fn(ops.fno3d_forward(sd, x), y).backward()
        opt_ops.step()

    def ops_forward():
        with torch.no_grad():
            ops.fno3d_forward(sd, x)
    variants["torch_ops"] = (ops_train, ops_forward)
    return variants


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_row(row, dev, windows, only, iters_override):
    variants = make_variants(row, dev)
    names = [n for n in ("hip", "torch_ops", "composed") if only is None or n in only]
    out = {"row": row["name"], "model": f"FNO3d{row['args']}", "input": list(row["shape"]), "variants": {}}
    for kind, idx in (("train", 0), ("forward", 1)):
        times = {n: [] for n in names}
        spent = {n: 0.0 for n in names}
        finished = {n: True for n in names}
        iters = {n: (row["composed_iters"] if n == "composed" else row["iters"]) for n in names}
        if iters_override:
            iters = {n: min(iters[n], iters_override) for n in names}
        for n in names:                                      # warm-up: plans, workspaces, the allocator, lazily compiled torch kernels
            t0 = time.perf_counter()
            window(variants[n][idx], 1 if n == "composed" else row["warmup"])
            spent[n] += time.perf_counter() - t0
        for _ in range(windows):
            for n in names:                                  # alternating: one window of each variant per round
                if n == "composed" and spent[n] > row["composed_limit_s"]:
                    finished[n] = False
                    continue
                t = window(variants[n][idx], iters[n])
                spent[n] += t * iters[n]
                times[n].append(t)
        for n in names:
            rec = out["variants"].setdefault(n, {})
            rec[kind] = {"ms_per_iteration": statistics.median(times[n]) * 1e3 if times[n] else None,
                         "windows_ms": [t * 1e3 for t in times[n]], "iterations_per_window": iters[n], "finished": finished[n]}
            if times[n]:
                rec[kind]["it_per_s"] = 1.0 / statistics.median(times[n])
    for n in names:                                          # peak memory of one training iteration, a round of its own
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if n == "composed" and not out["variants"][n]["train"]["finished"] and not out["variants"][n]["train"]["windows_ms"]:
            continue
        variants[n][0]()
        torch.cuda.synchronize()
        out["variants"][n]["train_peak_MiB"] = torch.cuda.max_memory_allocated() / 2**20
        out["variants"][n]["resident_before_MiB"] = base / 2**20
    hip = out["variants"].get("hip")
    if hip:
        for n in names:
            if n != "hip":
                for kind in ("train", "forward"):
                    t = out["variants"][n][kind]["ms_per_iteration"]
                    if t and hip[kind]["ms_per_iteration"]:
                        out["variants"][n][kind]["hip_speedup"] = t / hip[kind]["ms_per_iteration"]
    return out


def bench_head(dev, windows):
    """The head with last_activation alone, MLP(10, 1, 128) with GELU between at b P = 2^22 points: the fused kernels against the
    same two convolutions as channel einsums (torch materialises the (b, 128, P) hidden tensor)."""
    W, E, shape = 10, 128, (4, 10, 64, 64, 256)
    torch.manual_seed(0)
    head = fno.MLP(W, 1, E, activation=True).to(dev)
    x = torch.randn(*shape, device=dev, requires_grad=True)
    t = torch.randn(shape[0], 1, *shape[2:], device=dev)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in head.state_dict().items()}

    def ops_head(xin):
        h = torch.nn.functional.gelu(ops.conv1(xin, sd["mlp1.weight"], sd["mlp1.bias"]))
        return ops.conv1(h, sd["mlp2.weight"], sd["mlp2.bias"])

    def train(f, params):
        def run():
            for prm in params:
                prm.grad = None
            x.grad = None
            (f(x) * t).sum().backward()
        return run

    def fwd(f):
        def run():
            with torch.no_grad():
                f(x)
        return run
    fns = {"hip": (train(head, list(head.parameters())), fwd(head)), "torch_ops": (train(ops_head, list(sd.values())), fwd(ops_head))}
    out = {"row": "head_gelu", "model": "MLP(10, 1, 128, activation=True)", "input": list(shape), "variants": {}}
    for kind, idx in (("forward_backward", 0), ("forward", 1)):
        times = {n: [] for n in fns}
        for n in fns:
            window(fns[n][idx], 2)
        for _ in range(windows):
            for n in fns:
                times[n].append(window(fns[n][idx], 5))
        for n in fns:
            out["variants"].setdefault(n, {})[kind] = {"ms_per_iteration": statistics.median(times[n]) * 1e3,
                                                       "windows_ms": [v * 1e3 for v in times[n]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,2")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma list of variants (hip, torch_ops, composed)")
    ap.add_argument("--iters", type=int, default=0, help="cap on the iterations per window (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else None
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "timing": "wall clock per window, device-synchronised at both ends, variants alternating, median of the windows",
              "loss": "SobolevLoss(norm_order=0, relative=True, time_average=True) on the HIP loss kernels for all variants; Adam",
              "rows": []}
    for r in (int(k) for k in a.rows.split(",")):
        result["rows"].append(bench_head(dev, a.windows) if r == 3 else bench_row(ROWS[r], dev, a.windows, only, a.iters))
        print(json.dumps(result["rows"][-1]), flush=True)
        if a.out:                                            # after every row: a later row running out of time loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
