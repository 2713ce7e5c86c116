"""CPU-only checks of the data path: the plain-torch restatement tests/datasets_ops.py against every record the REFERENCE's
classes wrote into tests/golden/datasets.npz (bit for bit -- that licenses it as the oracle of the GPU tests at other
sizes), ``BatchLoader.plan()`` against ``torch.utils.data.DataLoader``, the normalisers' ``state_dict`` against the golden,
and the no-CPU-fallback rule.  No compute calls on a device."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import datasets_ops as ops
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("datasets.npz")


@pytest.fixture(scope="module")
def data(gold):
    return {f: torch.from_numpy(gold[f"data_{f}"]) for f in ops.FIELDS}


def test_module_imports_without_a_gpu():
    import torch_cfd_amd as tc
    from torch_cfd_amd import datasets, pipeline

    assert tc.BatchLoader is datasets.BatchLoader and tc.SpatioTemporalDataset is datasets.SpatioTemporalDataset
    assert tc.SpatioTemporalDatasetFixedTime is datasets.SpatioTemporalDatasetFixedTime
    for name in ("UnitGaussianNormalizer", "SpatialGaussianNormalizer", "add_grid_3d"):
        assert hasattr(datasets, name)
    assert callable(pipeline.train_batch_ns) and callable(pipeline.eval_epoch_ns)


def test_golden_inputs_are_the_seeded_draws(gold, data):
    again = ops.make_data(ops.GOLDEN_N, ops.GOLDEN_T, ops.GOLDEN_n)
    for f in ops.FIELDS:
        assert data[f].dtype == torch.float32 and torch.equal(data[f], again[f])


def test_restatement_reproduces_every_golden_record(gold, data):
    store = {}
    ops.golden_records(data, ops.np_record(store))
    names = sorted(k for k in gold.files if not k.startswith("data_"))
    assert names == sorted(store) and len(names) > 150
    for k in names:
        assert gold[k].dtype == store[k].dtype and gold[k].shape == store[k].shape, k
        assert np.array_equal(gold[k], store[k]), k


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_plan_equals_dataloader_index_batches(shuffle, drop_last):
    from torch_cfd_amd.datasets import BatchLoader

    N, B = 10, 4
    g_ref, g_new = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(1234)
    ref = DataLoader(range(N), batch_size=B, shuffle=shuffle, drop_last=drop_last, generator=g_ref)
    new = BatchLoader(range(N), B, shuffle=shuffle, drop_last=drop_last, generator=g_new)
    assert len(new) == len(ref)
    for _ in range(3):      # consecutive epochs keep in step too
        want = [b.tolist() for b in ref]
        plan = new.plan()
        assert [idx for idx, _ in plan] == want
        assert all(starts is None for _, starts in plan)
    assert torch.equal(g_ref.get_state(), g_new.get_state())
    if shuffle:             # a plain randperm under the same seed is ANOTHER order: the base seed is drawn first
        assert torch.randperm(N, generator=torch.Generator().manual_seed(1234)).tolist() != sum(
            [b.tolist() for b in DataLoader(range(N), batch_size=N, shuffle=True, generator=torch.Generator().manual_seed(1234))], [])


def test_plan_without_a_generator_follows_the_global_seed():
    from torch_cfd_amd.datasets import BatchLoader

    torch.manual_seed(7)
    want = [b.tolist() for b in DataLoader(range(10), batch_size=4, shuffle=True)]
    torch.manual_seed(7)
    assert [idx for idx, _ in BatchLoader(range(10), 4, shuffle=True).plan()] == want


class _Recorder(torch.utils.data.Dataset):
    """What DataLoader would fetch from a SpatioTemporalDataset: the index and the start drawn for it."""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, idx):
        return idx, self.ds.draw_start()


@pytest.mark.parametrize("shuffle", [False, True])
def test_plan_starts_are_the_numpy_draws_in_batch_order(data, shuffle):
    from torch_cfd_amd.datasets import BatchLoader, SpatioTemporalDataset

    big = {f: v.repeat(2, 3, 1, 1)[:10] for f, v in data.items()}        # 10 samples of 27 steps
    ds = SpatioTemporalDataset(big, n_samples=10, fields=list(ops.FIELDS), steps=3, out_steps=2, device="cpu")
    assert ds.total_steps == 27
    np.random.seed(99)
    ref = DataLoader(_Recorder(ds), batch_size=4, shuffle=shuffle, generator=torch.Generator().manual_seed(5))
    want = [(i.tolist(), s.tolist()) for i, s in ref]
    np.random.seed(99)
    plan = BatchLoader(ds, 4, shuffle=shuffle, generator=torch.Generator().manual_seed(5)).plan()
    assert plan == want
    np.random.seed(99)
    flat = [int(np.random.randint(0, 27 - (2 + 3 + 1))) for _ in range(10)]
    assert sum((s for _, s in plan), []) == flat
    fixed = SpatioTemporalDataset(big, n_samples=10, fields=list(ops.FIELDS), steps=3, out_steps=2, T_start=4, device="cpu")
    assert all(s == [4] * len(i) for i, s in BatchLoader(fixed, 4).plan())


@pytest.mark.parametrize("space", [False, True])
def test_normalizer_state_dict_matches_golden(gold, space):
    from torch_cfd_amd.datasets import SpatialGaussianNormalizer, UnitGaussianNormalizer

    cls = SpatialGaussianNormalizer if space else UnitGaussianNormalizer
    steps, To, n = ops.FIXED["steps"], ops.FIXED["out_steps"], ops.GOLDEN_n
    shapes = {"inp": (steps, n, 1) if space else (steps, n, n), "out": (n, n, 1) if space else (n, n, To)}
    for side in ("inp", "out"):
        state = {k: torch.from_numpy(gold[f"fixed_sp{int(space)}_{side}_{k}_vorticity"]) for k in ("mean", "std")}
        m = cls(device="cpu")
        assert list(m.state_dict()) == []
        m.load_state_dict(state)
        sd = m.state_dict()
        assert list(sd) == ["mean", "std"]
        for k in sd:
            assert sd[k].dtype == torch.float32 and tuple(sd[k].shape) == shapes[side] and torch.equal(sd[k], state[k])
        again = cls(device="cpu")
        again.load_state_dict(sd)
        assert torch.equal(again.mean, m.mean) and again.eps == 1e-7


def test_cpu_tensors_raise(data):
    from torch_cfd_amd import _lib
    from torch_cfd_amd.datasets import (SpatioTemporalDataset, SpatioTemporalDatasetFixedTime, UnitGaussianNormalizer,
                                        add_grid_3d)

    x = data["vorticity"]
    with pytest.raises(_lib.TcfdError):
        UnitGaussianNormalizer(device="cpu").fit_transform(x)
    m = UnitGaussianNormalizer(device="cpu")
    m.load_state_dict({"mean": x.mean(0), "std": x.std(0)})
    for call in (m.transform, m.inverse_transform, m):
        with pytest.raises(_lib.TcfdError):
            call(x)
    with pytest.raises(_lib.TcfdError):
        add_grid_3d(x.permute(0, 2, 3, 1))
    ds = SpatioTemporalDataset(dict(data), n_samples=4, fields=list(ops.FIELDS), steps=3, out_steps=2, device="cpu")
    with pytest.raises(_lib.TcfdError):
        ds.batch([0, 1], [0, 0])
    with pytest.raises(_lib.TcfdError):
        SpatioTemporalDatasetFixedTime(dict(data), n_samples=4, fields=list(ops.FIELDS), steps=3, out_steps=2, device="cpu")


def test_window_arguments_are_checked_on_the_host(data):
    from torch_cfd_amd.datasets import SpatioTemporalDataset

    ds = SpatioTemporalDataset(dict(data), n_samples=4, fields=list(ops.FIELDS), steps=3, out_steps=2, device="cpu")
    with pytest.raises(ValueError):
        ds.batch([0], [5])          # 5 + 3 + 2 > 9
    with pytest.raises(ValueError):
        ds.batch([0], [-1])
    with pytest.raises(IndexError):
        ds.batch([4], [0])
    with pytest.raises(ValueError):
        ds.batch([0, 1], [0])
    with pytest.raises(ValueError):
        SpatioTemporalDataset(dict(data), n_samples=7, fields=list(ops.FIELDS), device="cpu")
    with pytest.raises(KeyError):
        SpatioTemporalDataset(dict(data), n_samples=4, fields=["velocity"], device="cpu")


def test_abi_rejects_bad_arguments_without_touching_the_gpu():
    from torch_cfd_amd import _lib

    lib = _lib.load()
    for name in ("tcfd_data_window", "tcfd_data_fno3d_batch", "tcfd_data_affine", "tcfd_data_moments"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.tcfd_data_window(None, None, None, None, None, 1, 4, 9, 64, 65, 2, 0, 0, 0, None) == -1
    assert b"steps" in lib.tcfd_last_error()
    assert lib.tcfd_data_window(None, None, None, None, None, 1, 4, 4, 64, 3, 2, 0, 0, 0, None) == -1
    assert lib.tcfd_data_window(None, None, None, None, None, 1, 4, 9, 64, 3, 2, 0, 0, 5, None) == -1
    assert lib.tcfd_data_window(None, None, None, None, None, 0, 4, 9, 64, 3, 2, 0, 0, 0, None) == 0
    assert lib.tcfd_data_fno3d_batch(None, None, None, None, None, None, None, None, 5000, 6, 10, 8, 5, 0, 0, None) == -1
    assert lib.tcfd_data_affine(None, None, None, None, 10, 3, 1, 1e-7, 0, 0, 0, 0, None) == -1
    assert lib.tcfd_data_affine(None, None, None, None, 12, 3, 1, 1e-7, 2, 0, 0, 0, None) == -1
    assert lib.tcfd_data_moments(None, None, None, 0, 3, 1, 0, 0, None) == -1


@pytest.mark.parametrize("N", ops.STATS_N)
def test_float32_statistics_of_torch_itself_stay_inside_the_gpu_bound(N):
    """The bound tests/test_datasets_gpu.py sets for fitted float32 statistics, 2^-23 * max|x| around the float64 value,
    is one the reference's own float32 reductions meet on the same inputs: it asks nothing of the kernel that torch
    does not deliver."""
    x = ops.stats_input(N)
    x64 = x.double()
    bound = 2.0 ** -23 * x64.abs().max().item()
    for got, want in ((ops.unit_fit(x), (x64.mean(0), x64.std(0))),
                      (ops.spatial_fit(x), (x64.mean((0, -1)).unsqueeze(-1), x64.std((0, -1)).unsqueeze(-1)))):
        for g, w in zip(got, want):
            assert g.dtype == torch.float32 and (g.double() - w).abs().max().item() <= bound

