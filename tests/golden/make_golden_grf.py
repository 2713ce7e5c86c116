#!/usr/bin/env python
"""Generate tests/golden/grf.npz and tests/golden/fno_dataset.npz by IMPORTING THE REFERENCE (CPU only, deterministic).

Run only where the reference checkout is present (read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grf.py

``grf.npz``: outputs of the reference's ``GRF2d`` (fno/data_gen/grf.py, loaded by path) with ``device="cpu"`` -- the
sqrt_eig tables and samples for the cases tests/test_grf_host.py and tests/test_grf_gpu.py check.  The noise is not stored: it is
the seeded CPU stream, which the tests draw again (that the streams coincide is what the comparison confirms).

``fno_dataset.npz``: the batch loop of fno/data_gen/data_gen_fno.py:152-252 at a small size, restated from the reference's
own components (the driver module needs the argparse / logging plumbing of data_utils and is not importable here).  The
driver builds ``step_fn = IMEXStepper(order=2)`` and never hands it to the operator, so ``ns2d.step`` would call ``None``;
the evident intent ``solver=step_fn`` is restated.

Only data (inputs' parameters + the reference's outputs), no reference source, goes into the files.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "fno", "data_gen"))
HERE = os.path.dirname(os.path.abspath(__file__))

spec = importlib.util.spec_from_file_location("reference_grf", os.path.join(REF, "fno", "data_gen", "grf.py"))
reference_grf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(reference_grf)
GRF2d = reference_grf.GRF2d

N_MAX = 2048


def npy(t):
    return t.detach().cpu().numpy()


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)/1024:.1f} KiB")


def replicable(grf, n, seed):
    """data_gen_fno.py:195-204 for one sample: drawn at 2048^2, nearest-interpolated to n."""
    s = torch.stack([grf.sample(1, N_MAX, random_state=seed)])
    return F.interpolate(s, size=(n, n), mode="nearest").squeeze(1)[0]


def gen_grf():
    out = {}
    n = 64
    torch.set_default_dtype(torch.float64)
    # (alpha, tau) x normalize, one sample each; seeds 11 ..
    cases = []
    for i, (alpha, tau) in enumerate(((2.5, 7.0), (2.0, 3.0))):
        for normalize in (False, True):
            tag = f"a{alpha:g}_t{tau:g}_n{int(normalize)}"
            seed = 11 + len(cases)
            g = GRF2d(n=n, alpha=alpha, tau=tau, device="cpu", dtype=torch.float64, normalize=normalize)
            if not normalize:
                out[f"table_{tag}"] = npy(g.sqrt_eig)
            out[f"sample_{tag}"] = npy(g.sample(1, n, random_state=seed))
            cases.append((alpha, tau, int(normalize), seed))
    out["cases"] = np.array(cases)
    # two samples from ONE stream
    g = GRF2d(n=n, alpha=2.5, tau=7.0, device="cpu", dtype=torch.float64, normalize=True)
    out["bsz2_seed"] = np.array(5)
    out["bsz2_sample"] = npy(g.sample(2, n, random_state=5))
    # smoothing: noise drawn at 2048^2 and interpolated to the mesh
    g = GRF2d(n=n, alpha=2.5, tau=7.0, device="cpu", dtype=torch.float64, smoothing=True)
    out["smooth_seed"] = np.array(3)
    out["smooth_sample"] = npy(g.sample(1, n, random_state=3))
    # replicable init 2048 -> 64 (whole field) and 2048 -> 256 (every second point of the sub-sampled field: file size)
    g = GRF2d(n=n, alpha=2.5, tau=7.0, device="cpu", dtype=torch.float64)
    table = g.sqrt_eig.clone()
    out["rep_seed"] = np.array(42)
    out["rep64_sample"] = npy(replicable(g, 64, 42))
    out["table_2048_thin"] = npy(g.sqrt_eig[::97, ::89])     # the 2048 table the last call left behind, thinned
    g = GRF2d(n=256, alpha=2.5, tau=7.0, device="cpu", dtype=torch.float64, normalize=True)
    out["rep256_sample_thin"] = npy(replicable(g, 256, 42)[::2, ::2])
    assert torch.equal(table, GRF2d(n=n, alpha=2.5, tau=7.0, device="cpu").sqrt_eig)
    # an fp32 module under the float32 default (float32 table, complex64 product and transform), and the same noise and
    # table carried through the reference's own three operations in float64: the fp32 spread of the reference
    torch.set_default_dtype(torch.float32)
    g = GRF2d(n=n, alpha=2.5, tau=7.0, device="cpu", dtype=torch.float32)
    out["table_f32"] = npy(g.sqrt_eig)
    out["f32_seed"] = np.array(9)
    out["f32_sample"] = npy(g.sample(1, n, random_state=9))
    torch.random.manual_seed(9)
    coeff = torch.randn(1, 2, n, n, dtype=torch.float32)
    coeff = (coeff[:, 0] + 1j * coeff[:, 1]).to(torch.complex128)
    out["f32_exact"] = npy(torch.fft.ifftn(g.sqrt_eig.double() * coeff, dim=(-1, -2)).real)
    assert out["f32_sample"].dtype == np.float32 and out["table_f32"].dtype == np.float32
    torch.set_default_dtype(torch.float64)
    save("grf.npz", **out)


def gen_fno_dataset():
    import solvers
    from torch_cfd.equations import IMEXStepper, NavierStokes2DSpectral
    from torch_cfd.forcings import SinCosForcing
    from torch_cfd.grids import Grid

    solvers.tqdm = __import__("tqdm").tqdm
    torch.set_default_dtype(torch.float64)
    n, total_samples, batch_size, random_state, subsample = 64, 4, 2, 1127825, 2
    dt, warmup_steps, total_steps, record_every = 1e-3, 20, 40, 10
    visc, scale, diam, peak_wavenumber, alpha, tau = 1e-3, 0.1, 1.0, 4, 2.5, 7.0
    ns = n // subsample
    grid = Grid(shape=(n, n), domain=((0, diam), (0, diam)), device="cpu")
    forcing_fn = SinCosForcing(grid=grid, scale=scale, diam=diam, k=peak_wavenumber, vorticity=True)
    grf = GRF2d(n=n, alpha=alpha, tau=tau, normalize=False, device="cpu", dtype=torch.float64)
    step_fn = IMEXStepper(order=2)
    ns2d = NavierStokes2DSpectral(viscosity=visc, grid=grid, smooth=True, forcing_fn=forcing_fn, solver=step_fn)
    batches = []
    for i, idx in enumerate(range(0, total_samples, batch_size)):
        seeds = [random_state + idx + k for k in range(batch_size)]
        vort_init = torch.stack([grf.sample(1, N_MAX, random_state=s) for _, s in zip(range(batch_size), seeds)])
        vort_init = F.interpolate(vort_init, size=(n, n), mode="nearest").squeeze(1)
        vort_hat = torch.fft.rfft2(vort_init)
        for j in range(warmup_steps):
            vort_hat, _ = ns2d.step(vort_hat, dt)
        result = solvers.get_trajectory_imex(ns2d, vort_hat, dt, num_steps=total_steps, record_every_steps=record_every, pbar=False)
        for field, value in result.items():
            value = torch.fft.irfft2(value).real.cpu().to(torch.float32)
            result[field] = F.interpolate(value, size=(ns, ns), mode="bilinear")
        result["random_states"] = torch.as_tensor(seeds, dtype=torch.int32)
        batches.append(result)
    out = {k: npy(torch.cat([b[k] for b in batches])) for k in batches[0]}
    out["params"] = np.array([n, total_samples, batch_size, random_state, subsample, warmup_steps, total_steps, record_every])
    out["physics"] = np.array([dt, visc, scale, diam, peak_wavenumber, alpha, tau])
    save("fno_dataset.npz", **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["grf", "fno_dataset"]:
        globals()["gen_" + w]()
