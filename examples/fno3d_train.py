#!/usr/bin/env python
"""Train the FNO3d baseline the way examples/ex2_FNO3d_train_normalized.ipynb of the reference does, end to end and without any
download: a small decaying-turbulence (McWilliams) data set from this package's own solver at 64 x 64, the model
``FNO3d(32, 32, 5, 10, input_channel=10)`` on the first 10 recorded steps + the three coordinate channels, predicting the next 10,
relative L2 loss, Adam + OneCycleLR.

    python examples/fno3d_train.py [--samples 64] [--epochs 30] [--batch 4]

The model returns a tuple ``(prediction, None)``; the loop unpacks it (the reference's ``train_batch_ns`` hands ``model(a)``
straight to the loss, which its current fno3d.py no longer allows).  The data are not normalised (the notebook's
UnitGaussianNormalizer belongs to the data loaders, which this package does not ship): vorticity of O(1) trains as it is.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torch_cfd_amd import fno  # noqa: E402
from torch_cfd_amd.data_gen import generate_mcwilliams_dataset  # noqa: E402


def add_grid_3d(a: torch.Tensor) -> torch.Tensor:
    """(b, T_in, X, Y, T) -> (b, T_in + 3, X, Y, T): the coordinate channels x, y, t as ``linspace(0, 1)`` meshes
    (fno/datasets.py::add_grid_3d)."""
    b, _, X, Y, T = a.shape
    lin = lambda n: torch.linspace(0, 1, n, device=a.device, dtype=a.dtype)
    gx, gy, gt = torch.meshgrid(lin(X), lin(Y), lin(T), indexing="ij")
    return torch.cat([a, torch.stack([gx, gy, gt])[None].expand(b, -1, -1, -1, -1)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--test-samples", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--steps-in", type=int, default=10)
    ap.add_argument("--steps-out", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T_in, T_out, n = a.steps_in, a.steps_out, a.n
    total = a.samples + a.test_samples

    # ---- data: (samples, T_in + T_out, n, n) vorticity snapshots of decaying turbulence, computed in float64, stored float32
    torch.set_default_dtype(torch.float64)
    t0 = time.perf_counter()
    data = generate_mcwilliams_dataset(n, total, min(total, 16), 1e-3, warmup_steps=500, total_steps=100 * (T_in + T_out),
                                       record_every_steps=100, viscosity=1e-3, peak_wavenumber=4, random_state=0,
                                       dtype=torch.float32, cdtype=torch.complex64, device=dev)
    torch.set_default_dtype(torch.float32)
    w = data["vorticity"].to(dev)[:, : T_in + T_out]                       # (samples, T, n, n)
    print(f"data: vorticity {tuple(w.shape)} in {time.perf_counter() - t0:.1f} s, rms {w.square().mean().sqrt().item():.3f}")
    w = w.permute(0, 2, 3, 1).contiguous()                                 # (samples, n, n, T)
    # input: the first T_in steps as channels, repeated along the T_out output steps, + the coordinate channels
    inp = w[..., :T_in].permute(0, 3, 1, 2)[..., None].expand(-1, -1, -1, -1, T_out)
    inp = add_grid_3d(inp.contiguous())                                    # (samples, T_in + 3, n, n, T_out)
    out = w[..., T_in:].contiguous()                                       # (samples, n, n, T_out)
    tr_x, tr_y, te_x, te_y = inp[: a.samples], out[: a.samples], inp[a.samples:], out[a.samples:]

    torch.manual_seed(0)
    model = fno.FNO3d(32, 32, 5, 10, input_channel=T_in).to(dev)
    print(f"FNO3d: {sum(p.numel() for p in model.parameters())} parameters")
    loss_fn = fno.SobolevLoss(n_grid=n, norm_order=0, relative=True, time_average=True).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=a.lr)
    per_epoch = (a.samples + a.batch - 1) // a.batch
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=a.lr, total_steps=a.epochs * per_epoch, pct_start=0.2)

    def evaluate(x, y):
        with torch.no_grad():
            tot = 0.0
            for i in range(0, x.shape[0], a.batch):
                pred, _ = model(x[i:i + a.batch])
                tot += loss_fn(pred, y[i:i + a.batch]).item() * min(a.batch, x.shape[0] - i)
        return tot / x.shape[0]

    print(f"epoch  0: test rel-L2 {evaluate(te_x, te_y):.4f}")
    for epoch in range(1, a.epochs + 1):
        perm = torch.randperm(a.samples, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run = 0.0
        for i in range(0, a.samples, a.batch):
            idx = perm[i:i + a.batch]
            opt.zero_grad(set_to_none=True)
            pred, _ = model(tr_x[idx])                                     # the model returns (prediction, None)
            loss = loss_fn(pred, tr_y[idx])
            loss.backward()
            opt.step()
            sched.step()
            run += loss.item() * idx.numel()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if epoch % 5 and epoch != a.epochs:
            continue
        print(f"epoch {epoch:2d}: train rel-L2 {run / a.samples:.4f}  test rel-L2 {evaluate(te_x, te_y):.4f}  "
              f"{per_epoch / dt:.1f} it/s")


if __name__ == "__main__":
    main()
