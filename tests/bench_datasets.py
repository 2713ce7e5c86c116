#!/usr/bin/env python
"""Timing of one batch of the device-resident data sets (csrc/tcfd_data.hip) next to the same assembly in torch device ops
and next to the reference-style path (CPU tensors, ``Dataset.__getitem__`` per sample, ``DataLoader`` collate,
``.to(device)``), restated here.

    python tests/bench_datasets.py [--json profiles/datasets_bench.json] [--skip-cpu]

Per shape and data set class one batch is timed: device events around ``iters`` calls, after a warm-up, five regions per
variant with the variants ALTERNATING region by region inside this one process; the median and the spread (max - min) of
the five are reported.  The reference-style path is host work and is timed with the wall clock around one batch (device
synchronised), five times.  Bytes are the algorithmic ones computed from the shapes (fields read once, batch written
once), reported as a fraction of 8 TB/s.  ``moments_ms`` is one fit of ``UnitGaussianNormalizer`` statistics over the whole
input set (two passes).

No rate is fixed in advance.  The bar: at the 256 x 256 shape the one-launch batch takes less time than the torch-op
composition by more than the spread of the five regions (``bar_met``).  The 64 x 64 batches are launch-bound and only reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch.utils.data import DataLoader, Dataset

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from torch_cfd_amd import datasets as D  # noqa: E402

PEAK = 8e12
STEPS, OUT_STEPS, T_START = 10, 10, 5
# field shape, batch, calls per timed region (regions of 0.1 s and more)
SHAPES = (((256, 100, 64, 64), 4, 2000), ((256, 100, 64, 64), 32, 2000), ((64, 30, 256, 256), 32, 300))
MOMENTS_CALLS = 2000
FIELD = "vorticity"


def regions(variants, iters, warmup=2, count=5):
    """{name: [ms per call] * count}: the variants take turns region by region."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(count):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / iters)
    return times


def summary(ts):
    return {"median_ms": statistics.median(ts), "spread_ms": max(ts) - min(ts)}


class RefWindows(Dataset):
    """SpatioTemporalDataset of the reference on CPU tensors: a permuted view, sliced and cast per sample."""

    def __init__(self, field):
        self.x = field.permute(0, 2, 3, 1)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        s = T_START
        return ({FIELD: self.x[i, ..., s:s + STEPS].to(torch.float32)},
                {FIELD: self.x[i, ..., s + STEPS:s + STEPS + OUT_STEPS].to(torch.float32)})


class RefFixed(Dataset):
    """SpatioTemporalDatasetFixedTime of the reference on CPU tensors: the repeated input is built per sample."""

    def __init__(self, data_input, target):
        self.a, self.u = data_input, target
        n = target.shape[1]
        lin = lambda k: torch.linspace(0, 1, k)
        self.grid = torch.stack(torch.meshgrid(lin(n), lin(n), lin(OUT_STEPS), indexing="ij"))

    def __len__(self):
        return self.a.shape[0]

    def __getitem__(self, i):
        rep = self.a[i].unsqueeze(-1).repeat(1, 1, 1, OUT_STEPS)
        return {FIELD: torch.cat((self.grid, rep)).to(torch.float32)}, {FIELD: self.u[i].to(torch.float32)}


def host_path_ms(ds, batch, dev, count=5):
    times = []
    for _ in range(count + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inp, out = next(iter(DataLoader(ds, batch_size=batch)))
        a, u = inp[FIELD].to(dev), out[FIELD].to(dev)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del a, u
    return times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(os.path.dirname(HERE), "profiles", "datasets_bench.json"))
    ap.add_argument("--skip-cpu", action="store_true", help="leave the reference-style host path out")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for shape, batch, iters in SHAPES:
        N, T, n, _ = shape
        P = n * n
        gen = torch.Generator(device=dev).manual_seed(0)
        field = torch.randn(shape, generator=gen, device=dev) + 0.5
        idx = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:batch].tolist()
        idx_dev = torch.tensor(idx, device=dev)

        # ---- windows
        ds = D.SpatioTemporalDataset({FIELD: field}, n_samples=N, fields=[FIELD], steps=STEPS, out_steps=OUT_STEPS,
                                     T_start=T_START, device=dev)

        def win_hip():
            return ds.batch(idx)

        def win_ops():
            sel = field.index_select(0, idx_dev)
            a = sel[:, T_START:T_START + STEPS].permute(0, 2, 3, 1).contiguous()
            b = sel[:, T_START + STEPS:T_START + STEPS + OUT_STEPS].permute(0, 2, 3, 1).contiguous()
            return a, b

        got, want = win_hip(), win_ops()
        assert torch.equal(got[0][FIELD], want[0]) and torch.equal(got[1][FIELD], want[1])
        del got, want
        t = regions({"hip": win_hip, "torch_ops": win_ops}, iters)
        nbytes = 2 * 4 * batch * (STEPS + OUT_STEPS) * P
        hip, ops = summary(t["hip"]), summary(t["torch_ops"])
        row = {"dataset": "SpatioTemporalDataset", "field_shape": list(shape), "batch": batch, "hip": hip, "torch_ops": ops,
               "speedup_vs_torch_ops": ops["median_ms"] / hip["median_ms"], "algorithmic_bytes": nbytes,
               "fraction_of_8TBps": nbytes / (hip["median_ms"] * 1e-3) / PEAK,
               "bar_met": ops["median_ms"] - hip["median_ms"] > max(hip["spread_ms"], ops["spread_ms"])}
        if not args.skip_cpu:
            row["reference_style_host_path"] = summary(host_path_ms(RefWindows(field.cpu()), batch, dev))
        rows.append(row)
        print(json.dumps(row), flush=True)

        # ---- FNO3d batches (statistics fitted on the whole set)
        fx = D.SpatioTemporalDatasetFixedTime({FIELD: field}, n_samples=N, fields=[FIELD], T_start=T_START, steps=STEPS,
                                              out_steps=OUT_STEPS, inp_normalizer=True, out_normalizer=True, device=dev)
        del ds
        a_all, u_all = fx.data_input[FIELD], fx.data[FIELD]
        grid = fx.grid

        def fx_hip():
            return fx.batch(idx)

        def fx_ops():
            a = a_all.index_select(0, idx_dev).unsqueeze(-1).repeat(1, 1, 1, 1, OUT_STEPS)
            return torch.cat((grid.unsqueeze(0).repeat(batch, 1, 1, 1, 1), a), 1), u_all.index_select(0, idx_dev)

        got, want = fx_hip(), fx_ops()
        assert torch.equal(got[0][FIELD], want[0]) and torch.equal(got[1][FIELD], want[1])
        del got, want
        torch.cuda.empty_cache()
        t = regions({"hip": fx_hip, "torch_ops": fx_ops}, iters)
        nbytes = 4 * batch * P * (STEPS + OUT_STEPS + (3 + STEPS) * OUT_STEPS + OUT_STEPS)
        hip, ops = summary(t["hip"]), summary(t["torch_ops"])
        raw = field[:, T_START:T_START + STEPS].contiguous()
        tm = regions({"moments": lambda: D._hip_moments(raw, False, torch.float32)}, MOMENTS_CALLS)["moments"]
        mbytes = 2 * raw.numel() * 4
        row = {"dataset": "SpatioTemporalDatasetFixedTime", "field_shape": list(shape), "batch": batch,
               "batch_shape": [batch, 3 + STEPS, n, n, OUT_STEPS], "hip": hip, "torch_ops": ops,
               "speedup_vs_torch_ops": ops["median_ms"] / hip["median_ms"], "algorithmic_bytes": nbytes,
               "fraction_of_8TBps": nbytes / (hip["median_ms"] * 1e-3) / PEAK,
               "bar_met": ops["median_ms"] - hip["median_ms"] > max(hip["spread_ms"], ops["spread_ms"]),
               "moments": {**summary(tm), "set_shape": list(raw.shape), "algorithmic_bytes": mbytes,
                           "fraction_of_8TBps": mbytes / (statistics.median(tm) * 1e-3) / PEAK}}
        if not args.skip_cpu:
            row["reference_style_host_path"] = summary(host_path_ms(RefFixed(a_all.cpu(), u_all.cpu()), batch, dev))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fx, a_all, u_all, grid, raw, field
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
    print(f"wrote {args.json}")


if __name__ == "__main__":
    main()
