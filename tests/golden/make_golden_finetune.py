#!/usr/bin/env python
"""Generate tests/golden/finetune_*.npz -- the spectral refiner (fno/finetune.py::OutConvFT) -- by IMPORTING THE REFERENCE
and running it on the CPU in float64.  Run inside the build container only:

    python tests/golden/make_golden_finetune.py

The reference file does not run as committed, so this script works around two things before importing it:
  * fno/finetune.py does ``from data_gen.solvers import *``, and importing the ``data_gen`` package runs its __init__,
    which pulls in h5py (absent here): a bare ``data_gen`` package whose ``__path__`` is fno/data_gen is registered in
    sys.modules first, so only data_gen/solvers.py is executed;
  * fno/finetune.py uses ``fft_mesh_2d`` and ``spectral_laplacian_2d`` without importing them (construction raises
    NameError): both names are set on the imported ``fno.finetune`` module from ``torch_cfd.spectral``.
Nothing else of the reference is patched.  The default dtype is float64 during the run (as in the notebook), so the
reference's tables are float64.

Files (inputs are the smooth trajectories / forcings of tests/finetune_ops.py, which the tests rebuild; the files hold
outputs and parameters, no reference source):
  finetune_fwd_<case>.npz   w, w_t, residual of ``_fine_tune`` (b = 1, n = 64, t = 4) for four settings
  finetune_weights.npz      a head's convolution before and after ``_update_spectral_conv_weights`` (no RNG parity needed)
Deterministic: a rerun rewrites the files bit for bit.
"""
import math
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

pkg = types.ModuleType("data_gen")
pkg.__path__ = [os.path.join(REF, "fno", "data_gen")]
sys.modules["data_gen"] = pkg

import fno.finetune as ft  # noqa: E402
from torch_cfd.spectral import fft_mesh_2d, spectral_laplacian_2d  # noqa: E402

ft.fft_mesh_2d = fft_mesh_2d
ft.spectral_laplacian_2d = spectral_laplacian_2d

from finetune_ops import smooth_forcing, smooth_trajectory  # noqa: E402

N, NT = 64, 4
CASES = {
    # name: (diam, bdf_weight, dt, forcing)
    "notebook": (2 * math.pi, (0.5, 0.5), 1e-6, True),
    "d1_w01_dt3_f0": (1.0, (0, 1), 1e-3, False),
    "d1_w55_dt3_f1": (1.0, (0.5, 0.5), 1e-3, True),
    "d2pi_w01_dt6_f0": (2 * math.pi, (0, 1), 1e-6, False),
}


def main():
    torch.set_default_dtype(torch.float64)
    w = smooth_trajectory(1, N, NT)
    f = smooth_forcing(1, N)
    for name, (diam, weight, dt, forced) in CASES.items():
        head = ft.OutConvFT(8, 8, 3, n_grid=N, diam=diam, dt=dt, bdf_weight=weight, delta=1)
        kws = {"visc": head.visc, "laplacian": head.lap, "dealias_filter": head.dealias_filter, "dealias": head.dealias,
               "rfftmesh": (head.kx, head.ky), "diam": head.diam, "weight": head.bdf_weight}
        out = head._fine_tune(w.clone(), f.clone() if forced else None, **kws)
        np.savez_compressed(os.path.join(HERE, f"finetune_fwd_{name}.npz"),
                            **{k: v.numpy() for k, v in out.items()}, diam=diam, weight=np.array(weight), dt=dt,
                            forced=forced)
        print(name, {k: float(v.abs().max()) for k, v in out.items()})
    # weights: an old head (modes 4, 4, 2) with seeded weights -> fine-tuning head (modes 6, 6, 3)
    g = torch.Generator().manual_seed(0)
    old = ft.OutConvFT(4, 4, 2, n_grid=16, delta=1)
    for p in old.conv.parameters():
        p.data.copy_(torch.rand(p.shape, generator=g) - 0.5)
    new = ft.OutConvFT(4, 4, 2, n_grid=16, delta=1)
    torch.manual_seed(0)
    new._update_spectral_conv_weights(6, 6, 3, device="cpu", model=old)
    arrays = {}
    for k in range(4):
        arrays[f"old_weight{k}"] = old.conv.weight[k].data.numpy()
        arrays[f"old_bias{k}"] = old.conv.bias[k].data.numpy()
        arrays[f"new_weight{k}"] = new.conv.weight[k].data.numpy()
        arrays[f"new_bias{k}"] = new.conv.bias[k].data.numpy()
    arrays["state_dict_keys"] = np.array(list(new.state_dict().keys()))
    arrays["buffer_shapes"] = np.array([list(new.state_dict()[k].shape) for k in ("lap", "kx", "ky", "dealias_filter")])
    arrays["modes"] = np.array([new.mode_x, new.mode_y, new.mode_t])
    np.savez_compressed(os.path.join(HERE, "finetune_weights.npz"), **arrays)
    print("weights", sorted(arrays))


if __name__ == "__main__":
    main()
