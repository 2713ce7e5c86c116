#!/usr/bin/env python
"""Generate tests/golden/fno3d_*.npz -- the FNO3d baseline (fno/fno3d.py::FNO3d) -- by IMPORTING THE REFERENCE and running it on
the CPU in float32 (the model is float32 / complex64 only: its own .double() raises).  Run inside the build container only:

    python tests/golden/make_golden_fno3d.py

Per case of tests/fno3d_ops.py::CASES two files, each below 1 MiB:
  fno3d_<case>.npz        sd_<key>: the reference's state_dict (model built right after torch.manual_seed(SEED)); y: its output for
                          the input of fno3d_ops.case_input(case) (the tests rebuild input and target from there);
                          torch_version: the generator's torch build (the seeded-initialisation test needs the same one)
  fno3d_<case>_grad.npz   g_x and g_<key>: gradients of mean((y - target)^2) w.r.t. the input and every parameter
and fno3d_state_tables.npz: state_dict keys / shapes / dtypes of three constructor variants (lists of names, no values).
Complex tensors are stored as complex64 arrays.  Nothing of the reference is patched; the files hold its numbers, not its code.
Deterministic: a rerun rewrites the files bit for bit.
"""
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from fno.fno3d import FNO3d  # noqa: E402

import fno3d_ops as ops  # noqa: E402

# constructor variants of the key / shape / dtype table: positional (modes1, modes2, modes3, width) + keywords
VARIANTS = {
    "default": ((8, 8, 5, 20), {}),
    "notebook": ((32, 32, 5, 10), {"input_channel": 10}),
    "gelu_head_3layers": ((4, 3, 2, 16), {"input_channel": 4, "num_spectral_layers": 3, "last_activation": True,
                                          "channel_expansion": 32, "padding": 2}),
}


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    kib = os.path.getsize(path) / 1024
    print(f"{name}: {kib:.0f} KiB")
    assert kib < 1024, name


def main():
    torch.set_default_dtype(torch.float32)
    for case in ops.CASES:
        kw = ops.ctor_kwargs(case)
        torch.manual_seed(ops.SEED)
        model = FNO3d(**kw)
        x, target = ops.case_input(case)
        x = x.requires_grad_(True)
        y, none = model(x)
        assert none is None
        loss = ((y - target) ** 2).mean()
        names = [n for n, _ in model.named_parameters()]
        grads = torch.autograd.grad(loss, [x] + [p for _, p in model.named_parameters()])
        sd = {f"sd_{k}": v.detach().numpy() for k, v in model.state_dict().items()}
        save(f"fno3d_{case}.npz", y=y.detach().numpy(), torch_version=np.array(torch.__version__), **sd)
        save(f"fno3d_{case}_grad.npz", g_x=grads[0].numpy(), **{f"g_{n}": g.numpy() for n, g in zip(names, grads[1:])})
        # the restatement against the reference, for the record (tests/test_fno3d_host.py asserts it)
        sd_t = {k: v.detach() for k, v in model.state_dict().items()}
        y2, gx2, g2 = ops.loss_and_grads(sd_t, x.detach(), target, kw["padding"], kw["last_activation"])
        rel = lambda a, b: (torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1))).item()
        worst = max(rel(torch.view_as_real(g2[n]) if g2[n].is_complex() else g2[n],
                        torch.view_as_real(g) if g.is_complex() else g) for n, g in zip(names, grads[1:]))
        print(f"  {case}: fno3d_ops vs reference  y {rel(y2, y.detach()):.2e}  g_x {rel(gx2, grads[0]):.2e}  worst parameter gradient {worst:.2e}")
    table = {}
    for name, (args, kw) in VARIANTS.items():
        m = FNO3d(*args, **kw)
        table[name] = {"args": list(args), "kwargs": kw,
                       "state": [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()]}
    save("fno3d_state_tables.npz", table=np.array(json.dumps(table, sort_keys=True)))


if __name__ == "__main__":
    main()
