#!/usr/bin/env python
"""A few iterations of SFNO training against the data AND the equation: ``SobolevLoss + lambda * ResidualLoss`` on
decaying-turbulence snapshots generated on the spot by this package's own solver (unit square, 64 x 64, no download).

    python examples/sfno_residual_train.py [--iters 20] [--lam 1e-3]

The SFNO maps the first 10 recorded vorticity snapshots to the next 10.  ``ResidualLoss`` measures how far the predicted block
(b, n, n, T) is from solving  w_t + u . grad w = visc lap w  in Fourier space (stream function from the prediction itself);
its value and its gradient with respect to the prediction run on the fused kernels of csrc/tcfd_residual.hip.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torch_cfd_amd import fno  # noqa: E402
from torch_cfd_amd.data_gen import generate_mcwilliams_dataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lam", type=float, default=1e-3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, T, visc, dt, every = a.n, 10, 1e-3, 1e-3, 20

    torch.set_default_dtype(torch.float64)
    data = generate_mcwilliams_dataset(n, a.samples, min(a.samples, 16), dt, warmup_steps=200, total_steps=every * 2 * T,
                                       record_every_steps=every, viscosity=visc, diam=1.0, peak_wavenumber=4, random_state=0,
                                       dtype=torch.float32, cdtype=torch.complex64, device=dev)
    torch.set_default_dtype(torch.float32)
    w = data["vorticity"].to(dev)[:, : 2 * T].permute(0, 2, 3, 1).contiguous()       # (samples, n, n, 2 T), time last
    x, y = w[..., :T].contiguous(), w[..., T:].contiguous()

    torch.manual_seed(0)
    model = fno.SFNO(16, 16, 5, width=10, num_spectral_layers=2).to(dev)
    data_loss = fno.SobolevLoss(n_grid=n, norm_order=0, relative=True).to(dev)
    pde_loss = fno.ResidualLoss(batch_size=a.batch, visc=visc, n_grid=n, n_t=T, delta_t=dt * every)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    with torch.no_grad():
        print(f"residual of the data itself: {pde_loss(y[: a.batch]).item():.4e}")
    for it in range(a.iters):
        idx = torch.randint(0, a.samples, (a.batch,), device=dev)
        opt.zero_grad(set_to_none=True)
        pred = model(x[idx])
        l_data, l_pde = data_loss(pred, y[idx]), pde_loss(pred)
        (l_data + a.lam * l_pde).backward()
        opt.step()
        if it % 5 == 0 or it == a.iters - 1:
            print(f"iter {it:3d}: relative L2 {l_data.item():.4f}   residual {l_pde.item():.4e}")


if __name__ == "__main__":
    main()
