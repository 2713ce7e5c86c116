"""CPU-only checks of the GRF2d sampler: the sqrt_eig tables against the reference's (bit for bit), the plain-torch
restatement tests/grf_ops.py of the kernel's fold formula against every sample the reference recorded in
tests/golden/grf.npz (which also confirms that the seeded CPU noise streams coincide), the noise chunk schedule, the seed
rule and the argument checks.  No compute calls on a device."""
import numpy as np
import pytest
import torch

import grf_ops as G
from conftest import load_golden, rel_l2

N = 64
N_MAX = 2048
# closed-form operator in float64: the project's convention (tests/test_fvm_grad_host.py: 1e-12 / 1e-13); measured ~3e-16
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return load_golden("grf.npz")


def _module(**kw):
    from torch_cfd_amd.grf import GRF2d

    return GRF2d(device="cpu", **kw)


def _cases(gold):
    for alpha, tau, normalize, seed in gold["cases"]:
        yield float(alpha), float(tau), bool(normalize), int(seed), f"a{alpha:g}_t{tau:g}_n{int(normalize)}"


def test_package_exports_grf2d():
    import torch_cfd_amd as tc
    from torch_cfd_amd.grf import GRF2d

    assert tc.GRF2d is GRF2d


def test_sqrt_eig_tables_are_bit_equal(gold):
    torch.set_default_dtype(torch.float64)
    for alpha, tau, normalize, _, tag in _cases(gold):
        if normalize:
            continue
        g = _module(n=N, alpha=alpha, tau=tau, dtype=torch.float64)
        assert g.sqrt_eig.dtype == torch.float64 and np.array_equal(g.sqrt_eig.numpy(), gold[f"table_{tag}"])
    g = _module(n=N, alpha=2.5, tau=7.0, dtype=torch.float64)
    assert np.array_equal(g._table(N_MAX)[::97, ::89].numpy(), gold["table_2048_thin"])
    # tables are kept per size: the one of the module's own n is still the one it was built with
    assert np.array_equal(g.sqrt_eig.numpy(), gold["table_a2.5_t7_n0"]) and g.sqrt_eig.shape == (N, N)
    torch.set_default_dtype(torch.float32)
    g = _module(n=N, alpha=2.5, tau=7.0, dtype=torch.float32)
    assert g.sqrt_eig.dtype == torch.float32 and np.array_equal(g.sqrt_eig.numpy(), gold["table_f32"])


def test_attributes_follow_the_reference():
    g = _module(n=32, alpha=2, tau=3, normalize=True, smoothing=True)
    assert (g.dim, g.n, g.alpha, g.tau, g.normalize, g.smoothing, g.max_mesh_size) == (2, 32, 2, 3, True, True, 2048)
    assert g.dtype == torch.float and g.device == "cpu"


def test_fold_formula_reproduces_the_reference_samples(gold):
    torch.set_default_dtype(torch.float64)
    errs = {}
    for alpha, tau, normalize, seed, tag in _cases(gold):
        table = torch.from_numpy(gold[f"table_a{alpha:g}_t{tau:g}_n0"])
        got = G.field(G.fold_spectrum(G.seeded_noise(seed, 1, N), table, N, normalize))
        errs[tag] = rel_l2(got, gold[f"sample_{tag}"])
    table = torch.from_numpy(gold["table_a2.5_t7_n0"])
    got = G.field(G.fold_spectrum(G.seeded_noise(int(gold["bsz2_seed"]), 2, N), table, N, True))
    assert got.shape == (2, N, N)
    errs["bsz2"] = rel_l2(got, gold["bsz2_sample"])
    noise = G.smoothed(G.seeded_noise(int(gold["smooth_seed"]), 1, N_MAX), N)
    errs["smooth"] = rel_l2(G.field(G.fold_spectrum(noise, table, N)), gold["smooth_sample"])
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_alias_fold_reproduces_the_replicable_init(gold):
    from torch_cfd_amd.grf import sqrt_eig_table

    torch.set_default_dtype(torch.float64)
    table = sqrt_eig_table(N_MAX, 2.5, 7.0)
    noise = G.seeded_noise(int(gold["rep_seed"]), 1, N_MAX)
    e64 = rel_l2(G.field(G.fold_spectrum(noise, table, 64))[0], gold["rep64_sample"])
    e256 = rel_l2(G.field(G.fold_spectrum(noise, table, 256, normalize=True))[0, ::2, ::2], gold["rep256_sample_thin"])
    print(e64, e256)
    assert e64 <= TOL and e256 <= TOL


def test_fp32_restatement_within_the_reference_spread(gold):
    """fp32 against the float64 result at the same fp32 noise and table: within twice the reference's own fp32 spread."""
    noise = G.seeded_noise(int(gold["f32_seed"]), 1, N, torch.float32)
    table = torch.from_numpy(gold["table_f32"])
    exact = torch.from_numpy(gold["f32_exact"])
    assert rel_l2(G.field(G.fold_spectrum(noise.double(), table.double(), N)), exact) <= TOL
    spread = rel_l2(gold["f32_sample"], exact)
    assert 1e-9 < spread < 1e-4
    got = G.field(G.fold_spectrum(noise, table, N))
    assert got.dtype == torch.float32 and rel_l2(got, exact) <= 2 * spread


def test_noise_chunks_cover_every_sample_once_under_the_cap():
    from torch_cfd_amd.grf import NOISE_BYTES_CAP, noise_chunks

    assert NOISE_BYTES_CAP == 1 << 30
    for count, n0, itemsize, cap in ((1, 64, 8, 1 << 30), (37, 2048, 8, 1 << 30), (256, 256, 8, 1 << 30), (16, 2048, 8, 1 << 30),
                                     (100, 2048, 4, 1 << 30), (7, 64, 8, 3 * 2 * 64 * 64 * 8), (5, 64, 8, 100), (0, 64, 8, 1 << 30)):
        pieces = noise_chunks(count, n0, itemsize, cap)
        covered = [i for start, c in pieces for i in range(start, start + c)]
        assert covered == list(range(count))
        per_sample = 2 * n0 * n0 * itemsize
        assert all(c >= 1 and (c * per_sample <= cap or c == 1) for _, c in pieces)
    assert noise_chunks(37, 2048, 8) == [(0, 16), (16, 16), (32, 5)]


def test_pieces_of_one_stream_continue_it():
    """sample(bsz) draws randn(bsz, 2, n, n) from one stream; staging it in pieces must not change a value."""
    g = _module(n=N, dtype=torch.float64)
    whole = G.seeded_noise(4, 5, N)
    gen = torch.Generator().manual_seed(4)
    parts = torch.cat([g._draw([gen], c, N) for c in (2, 1, 2)])
    assert torch.equal(parts, whole)
    gens = [torch.Generator().manual_seed(s) for s in (7, 8, 9, 10, 11)]
    each = g._draw(gens, 1, N)
    assert all(torch.equal(each[i:i + 1], G.seeded_noise(7 + i, 1, N)) for i in range(5))


def test_fno_dataset_seed_rule():
    from torch_cfd_amd.data_gen import fno_sample_seeds

    assert fno_sample_seeds(1127825, 4, 3) == [1127829, 1127830, 1127831]


def test_argument_checks():
    from torch_cfd_amd._lib import TcfdError

    g = _module(n=N, dtype=torch.float64)
    with pytest.raises(TcfdError):
        g.sample(1)
    with pytest.raises(TcfdError):
        g.sample_hat([0], N)
    with pytest.raises(TcfdError):
        g(torch.zeros(2, 1, N, N))
    with pytest.raises(NotImplementedError, match="divides n0"):
        g.sample_hat([0], 48, n0=N, device="cuda")
    with pytest.raises(NotImplementedError):
        _module(dim=3)


def test_c_abi_rejects_bad_sizes_without_touching_the_gpu():
    import torch_cfd_amd as tc

    lib = tc._lib.load()
    assert lib.tcfd_grf_spectrum_workspace_bytes(3, 64, 0) == 0
    assert lib.tcfd_grf_spectrum_workspace_bytes(3, 64, 1) == 3 * (-(-64 * 33 // 256) + 1) * 8
    assert lib.tcfd_grf_spectrum(None, None, None, 1, 100, 64, tc._lib.TCFD_C128, 0, None, 0, None) == -1
    assert b"divide" in lib.tcfd_last_error()
    assert lib.tcfd_grf_spectrum(None, None, None, 1, 64, 64, 5, 0, None, 0, None) == -1
    assert lib.tcfd_grf_spectrum(None, None, None, 1, 64, 64, tc._lib.TCFD_C128, 0, None, 0, None) == -1
    assert b"null" in lib.tcfd_last_error()
