#!/usr/bin/env python
"""The loop of examples/ex2_FNO3d_train_normalized.ipynb of the reference, run from a ``.pt`` data set through this package's
device-resident data path: ``SpatioTemporalDatasetFixedTime`` (normalisers fitted on the train split, applied to the test
split), ``BatchLoader``, ``train_batch_ns`` and ``eval_epoch_ns``.

    python examples/fno3d_train_normalized.py [--data data.pt] [--samples 64] [--epochs 30] [--batch 4]

Without ``--data`` (or when the file does not exist yet) a small decaying-turbulence (McWilliams) data set is computed by
this package's own solver at 64 x 64 and saved there first; any ``.pt`` dict with a ``vorticity`` field (N, T, n, n) of at
least ``steps-in + steps-out`` recorded steps works, such as the ones ``data_gen.generate_*_dataset`` write.

The fields stay on the device; every batch ``(b, 3 + steps-in, n, n, steps-out)`` is one kernel launch over them.  The model
predicts the NORMALISED target; ``train_batch_ns`` decodes prediction and target with the output normaliser before the
relative L2 loss, as the notebook does.
"""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torch_cfd_amd import fno  # noqa: E402
from torch_cfd_amd.data_gen import generate_mcwilliams_dataset  # noqa: E402
from torch_cfd_amd.datasets import BatchLoader, SpatioTemporalDatasetFixedTime  # noqa: E402
from torch_cfd_amd.pipeline import eval_epoch_ns, train_batch_ns  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help=".pt data set; computed and saved there when missing")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--test-samples", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--steps-in", type=int, default=10)
    ap.add_argument("--steps-out", type=int, default=10)
    ap.add_argument("--modes", type=int, default=5)
    ap.add_argument("--width", type=int, default=10)
    ap.add_argument("--warmup-steps", type=int, default=500)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T_in, T_out = a.steps_in, a.steps_out
    total = a.samples + a.test_samples
    path = a.data or os.path.join(tempfile.gettempdir(), f"mcwilliams_{a.n}_{total}_{T_in + T_out}.pt")

    if not os.path.exists(path):      # computed in float64, stored float32, as the reference's drivers do
        torch.set_default_dtype(torch.float64)
        t0 = time.perf_counter()
        generate_mcwilliams_dataset(a.n, total, min(total, 16), 1e-3, warmup_steps=a.warmup_steps, total_steps=100 * (T_in + T_out),
                                    record_every_steps=100, viscosity=1e-3, peak_wavenumber=4, random_state=0,
                                    dtype=torch.float32, cdtype=torch.complex64, device=dev, path=path)
        torch.set_default_dtype(torch.float32)
        print(f"data: wrote {path} in {time.perf_counter() - t0:.1f} s")

    kw = dict(fields=["vorticity"], T_start=0, steps=T_in, out_steps=T_out, device=dev)
    train = SpatioTemporalDatasetFixedTime(path, n_samples=a.samples, train=True, inp_normalizer=True, out_normalizer=True, **kw)
    test = SpatioTemporalDatasetFixedTime(path, n_samples=a.test_samples, train=False, inp_normalizer=train.inp_normalizer,
                                          out_normalizer=train.out_normalizer, **kw)
    n = train.data["vorticity"].shape[1]
    print(f"train {tuple(train.data_input['vorticity'].shape)} -> {tuple(train.data['vorticity'].shape)}, test {len(test)} samples; "
          f"output std in [{train.out_normalizer['vorticity'].std.min().item():.3f}, "
          f"{train.out_normalizer['vorticity'].std.max().item():.3f}]")
    gen = torch.Generator().manual_seed(0)
    train_loader = BatchLoader(train, a.batch, shuffle=True, generator=gen)
    test_loader = BatchLoader(test, a.batch)

    torch.manual_seed(0)
    model = fno.FNO3d(a.modes, a.modes, min(a.modes, T_out // 2 + 1), a.width, input_channel=T_in).to(dev)
    print(f"FNO3d: {sum(p.numel() for p in model.parameters())} parameters")
    loss_fn = fno.SobolevLoss(n_grid=n, norm_order=0, relative=True, time_average=True).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=a.lr)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=a.lr, total_steps=a.epochs * len(train_loader), pct_start=0.2)
    normalizer = train.out_normalizer

    print(f"epoch  0: test rel-L2 {eval_epoch_ns(model, loss_fn, test_loader, dev, normalizer=normalizer):.4f}")
    for epoch in range(1, a.epochs + 1):
        model.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run, seen = torch.zeros((), device=dev), 0
        for batch in train_loader:
            loss = train_batch_ns(model, loss_fn, batch, opt, dev, normalizer=normalizer)
            sched.step()
            b = batch[1]["vorticity"].shape[0]
            run += loss.detach() * b
            seen += b
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if epoch % 5 and epoch != a.epochs:
            continue
        print(f"epoch {epoch:2d}: train rel-L2 {run.item() / seen:.4f}  "
              f"test rel-L2 {eval_epoch_ns(model, loss_fn, test_loader, dev, normalizer=normalizer):.4f}  "
              f"{len(train_loader) / dt:.1f} it/s")


if __name__ == "__main__":
    main()
