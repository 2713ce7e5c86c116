"""GPU checks of the GRF2d sampler (tcfd_grf_spectrum) and of generate_fno_dataset: parity with the reference's recorded
samples (tests/golden/grf.npz) and with the plain-torch restatement tests/grf_ops.py (validated against the same records on
the CPU, tests/test_grf_host.py), run-to-run determinism, the normalisation, and the data set against the reference's loop
(tests/golden/fno_dataset.npz)."""
import numpy as np
import pytest
import torch

import grf_ops as G
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

N = 64
N_MAX = 2048
TOL = 1e-12   # float64 closed-form operator, as tests/test_grf_host.py


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_golden("grf.npz")


def scaled_err(a, b, scale_of):
    """||a - b|| / ||scale_of||: the error of a difference of larger terms against the terms that cancel
    (tests/test_ns2d_gpu.py)."""
    a, b, s = (torch.as_tensor(x).to("cpu", torch.complex128) for x in (a, b, scale_of))
    return (torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(s.reshape(-1))).item()


def _module(dev, **kw):
    import torch_cfd_amd as tc

    return tc.GRF2d(device=dev, **kw)


def _irfft2(hat):
    import torch_cfd_amd as tc

    return tc.fft_plan(hat.shape[-2], hat.dtype, hat.device).irfft2(hat)


def test_samples_match_the_reference(dev, gold):
    torch.set_default_dtype(torch.float64)
    errs = {}
    for alpha, tau, normalize, seed in gold["cases"]:
        tag = f"a{alpha:g}_t{tau:g}_n{int(normalize)}"
        g = _module(dev, n=N, alpha=float(alpha), tau=float(tau), dtype=torch.float64, normalize=bool(normalize))
        s = g.sample(1, N, random_state=int(seed))
        assert s.shape == (1, N, N) and s.dtype == torch.float64 and s.device.type == "cuda"
        errs[tag] = rel_l2(s, gold[f"sample_{tag}"])
        hat = g.sample_hat([int(seed)], N)
        assert hat.shape == (1, N, N // 2 + 1) and hat.dtype == torch.complex128
        errs[tag + "_hat"] = rel_l2(_irfft2(hat), gold[f"sample_{tag}"])
        errs[tag + "_fwd"] = rel_l2(g(torch.zeros(1, 3, N, N, device=dev), random_state=int(seed)), gold[f"sample_{tag}"])
    g = _module(dev, n=N, alpha=2.5, tau=7.0, dtype=torch.float64, normalize=True)
    s = g.sample(2, random_state=int(gold["bsz2_seed"]))
    assert s.shape == (2, N, N)
    errs["bsz2"] = rel_l2(s, gold["bsz2_sample"])
    g = _module(dev, n=N, alpha=2.5, tau=7.0, dtype=torch.float64, smoothing=True)
    errs["smooth"] = rel_l2(g.sample(1, random_state=int(gold["smooth_seed"])), gold["smooth_sample"])
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_replicable_init_matches_the_reference(dev, gold):
    torch.set_default_dtype(torch.float64)
    seed = int(gold["rep_seed"])
    g = _module(dev, n=N, alpha=2.5, tau=7.0, dtype=torch.float64)
    e64 = rel_l2(_irfft2(g.sample_hat([seed], N, n0=N_MAX))[0], gold["rep64_sample"])
    # the module is used at 2048 and then again at its own size: tables are kept per size
    assert rel_l2(g.sample(1, random_state=11), gold["sample_a2.5_t7_n0"]) <= TOL
    g = _module(dev, n=256, alpha=2.5, tau=7.0, dtype=torch.float64, normalize=True)
    e256 = rel_l2(_irfft2(g.sample_hat([seed], 256, n0=N_MAX))[0, ::2, ::2], gold["rep256_sample_thin"])
    print(e64, e256)
    assert e64 <= TOL and e256 <= TOL
    with pytest.raises(NotImplementedError, match="divides n0"):
        g.sample_hat([seed], 96, n0=N_MAX)


def test_fp32_within_the_reference_spread(dev, gold):
    """fp32 module under the float32 default (float32 table): against the float64 result at the same fp32 noise and table,
    within twice the reference's own fp32 spread (the rule of test_restatement_fp32_gradient_against_the_reference)."""
    torch.set_default_dtype(torch.float32)
    g = _module(dev, n=N, alpha=2.5, tau=7.0, dtype=torch.float32)
    got = g.sample(1, random_state=int(gold["f32_seed"]))
    assert got.dtype == torch.float32
    exact = torch.from_numpy(gold["f32_exact"])
    spread = rel_l2(gold["f32_sample"], exact)
    err = rel_l2(got, exact)
    print(err, spread)
    assert 1e-9 < spread < 1e-4
    assert err <= 2 * spread


@pytest.mark.parametrize("n0,n,bsz,normalize", [(256, 256, 2, False), (1024, 1024, 2, True), (N_MAX, 256, 3, True),
                                                 (N_MAX, 256, 3, False)])
def test_spectrum_matches_the_restatement(dev, n0, n, bsz, normalize):
    torch.set_default_dtype(torch.float64)
    seeds = [100 + i for i in range(bsz)]
    g = _module(dev, n=n, alpha=2.5, tau=7.0, dtype=torch.float64, normalize=normalize)
    hat = g.sample_hat(seeds, n, n0=n0)
    noise = torch.cat([G.seeded_noise(s, 1, n0) for s in seeds]).to(dev)
    want = G.fold_spectrum(noise, g._table(n0).to(dev), n, normalize)
    err = rel_l2(hat.cpu(), want.cpu())
    print(err)
    assert hat.shape == want.shape and err <= TOL
    if n0 == n:
        # the formula's own zeros: DC (the table's), and Im of the self-conjugate modes
        assert torch.all(hat[:, 0, 0] == 0)
        assert torch.all(hat[:, [0, n // 2, 0, n // 2], [0, 0, n // 2, n // 2]].imag == 0)


@pytest.mark.parametrize("normalize", [False, True])
def test_two_runs_give_the_same_bits(dev, normalize):
    torch.set_default_dtype(torch.float64)
    g = _module(dev, n=256, alpha=2.5, tau=7.0, dtype=torch.float64, normalize=normalize)
    for n0 in (256, N_MAX):
        a = g.sample_hat([1, 2, 3], 256, n0=n0)
        b = g.sample_hat([1, 2, 3], 256, n0=n0)
        assert torch.equal(a, b)
    assert torch.equal(g.sample(3, random_state=8), g.sample(3, random_state=8))
    # a sample does not depend on what it is batched with
    assert torch.equal(g.sample_hat([1, 2, 3], 256)[1:2], g.sample_hat([2], 256))


def test_normalize_and_transform_consistency(dev):
    import torch_cfd_amd as tc

    torch.set_default_dtype(torch.float64)
    n = 256
    g = _module(dev, n=n, alpha=2.0, tau=3.0, dtype=torch.float64, normalize=True)
    s = g.sample(4, random_state=21)
    norms = torch.linalg.norm(s / n, dim=(-1, -2))
    assert (norms - 1).abs().max().item() <= TOL, norms
    gens = g.sample_hat([21, 22], n)
    plan = tc.fft_plan(n, torch.complex128, dev)
    assert rel_l2(plan.rfft2(plan.irfft2(gens)), gens) <= TOL
    # sample(bsz) is the irfft2 of the spectrum of the same stream: its first sample is sample_hat of that seed
    assert rel_l2(plan.rfft2(s[:1]), g.sample_hat([21], n)) <= TOL


def test_staging_in_pieces_does_not_change_a_sample(dev, monkeypatch):
    from torch_cfd_amd import grf as grf_mod

    torch.set_default_dtype(torch.float64)
    g = _module(dev, n=N, alpha=2.5, tau=7.0, dtype=torch.float64, normalize=True)
    whole_s, whole_h = g.sample(5, random_state=2), g.sample_hat(list(range(5)), N)
    real_chunks = grf_mod.noise_chunks
    monkeypatch.setattr(grf_mod, "noise_chunks", lambda count, n0, itemsize: real_chunks(count, n0, itemsize, 2 * 2 * N * N * 8))
    assert torch.equal(g.sample(5, random_state=2), whole_s) and torch.equal(g.sample_hat(list(range(5)), N), whole_h)


def _dataset(dev, g, **kw):
    from torch_cfd_amd.data_gen import generate_fno_dataset

    n, total, batch, seed, sub, warm, steps, every = (int(v) for v in g["params"])
    dt, visc, scale, diam, k, alpha, tau = (float(v) for v in g["physics"])
    args = dict(viscosity=visc, diam=diam, scale=scale, peak_wavenumber=k, alpha=alpha, tau=tau, replicable_init=True,
                random_state=seed, subsample=sub, device=dev)
    args.update(kw)
    batch = args.pop("batch_size", batch)
    return generate_fno_dataset(n, total, batch, dt, warm, steps, every, **args)


def test_fno_dataset_golden(dev, tmp_path):
    """The loop of fno/data_gen/data_gen_fno.py:152-252 (SinCos forcing, IMEX order 2, replicable GRF initial condition,
    warm-up, get_trajectory_imex, irfft2 -> float32 -> bilinear subsample, random_states) against the same loop run with the
    imported reference's components; tolerances and structure of test_kolmogorov_dataset_golden."""
    torch.set_default_dtype(torch.float64)
    g = load_golden("fno_dataset.npz")
    n, total, batch, seed, sub, warm, steps, every = (int(v) for v in g["params"])
    path = str(tmp_path / "fno.pt")
    stats = {}
    data = _dataset(dev, g, path=path, stats=stats)
    n_rec = len(range(0, steps, every))
    assert sorted(data) == ["random_states", "residual", "stream", "vort_t", "vorticity"]
    assert torch.equal(data["random_states"], torch.from_numpy(g["random_states"])) and data["random_states"].dtype == torch.int32
    assert data["random_states"].tolist() == [seed + i for i in range(total)]
    for k in ("vorticity", "stream", "vort_t", "residual"):
        assert data[k].shape == g[k].shape == (total, n_rec, n // sub, n // sub) and data[k].dtype == torch.float32
    errs = dict(vorticity=rel_l2(data["vorticity"], g["vorticity"]), stream=rel_l2(data["stream"], g["stream"]),
                vort_t=scaled_err(data["vort_t"], torch.from_numpy(g["vort_t"]), torch.from_numpy(g["vorticity"]) / 1e-3),
                residual=scaled_err(data["residual"], torch.from_numpy(g["residual"]), torch.from_numpy(g["vort_t"])))
    print(errs)
    assert errs["vorticity"] < 1e-6 and errs["stream"] < 1e-6
    assert errs["vort_t"] < 1e-6
    assert errs["residual"] < 1e-3
    saved = torch.load(path)
    assert all(torch.equal(saved[k], data[k]) for k in data)
    assert stats["samples"] == total and stats["stepping_s"] > 0


def test_fno_dataset_batching_and_extra_vars(dev, tmp_path):
    torch.set_default_dtype(torch.float64)
    g = load_golden("fno_dataset.npz")
    by2 = _dataset(dev, g)
    by4 = _dataset(dev, g, batch_size=4)
    # seeds follow the global sample index: the batch size does not change a sample
    assert all(torch.equal(by2[k], by4[k]) for k in by2)
    assert not torch.equal(by2["vorticity"][1], by2["vorticity"][2])
    path = str(tmp_path / "fno_plain.pt")
    plain = _dataset(dev, g, extra_vars=False, path=path)
    assert torch.equal(plain["vorticity"], by2["vorticity"]) and torch.equal(plain["random_states"], by2["random_states"])
    assert all(plain[k].numel() == 0 for k in ("vort_t", "stream", "residual"))
    saved = torch.load(path)
    assert sorted(saved) == sorted(plain) and all(saved[k].numel() == 0 for k in ("vort_t", "stream", "residual"))
    # without the replicable init the field is drawn at n itself: another flow
    assert not torch.equal(_dataset(dev, g, replicable_init=False)["vorticity"], by2["vorticity"])
