"""GPU checks of the data path (torch-cfd_amd/datasets.py, pipeline.py, csrc/tcfd_data.hip).

Windows, FNO3d batches and the two affine transforms only copy, cast and apply correctly rounded single operations, so
they are compared BIT FOR BIT with tests/golden/datasets.npz (written by the reference's classes) or with
tests/datasets_ops.py run on the CPU on the same inputs (tests/test_datasets_host.py shows that it reproduces the golden
file bit for bit).  The fitted statistics are accumulated in fp64 in another order than torch's, so they carry a bound:

* float32 statistics: |stat - float64 CPU value| <= 2^-23 * max|x| -- one rounding to float32 of an fp64-accumulated
  value (2^-24 relative to a value below max|x|), with a factor 2 of room; torch's own float32 reductions stay inside it
  for these inputs (tests/test_datasets_host.py::test_float32_statistics_of_torch_itself_stay_inside_the_gpu_bound);
* float64 statistics: <= N * 2^-52 * max|x|;
* against the golden file's statistics (which carry the reference's own error): twice that.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

import datasets_ops as ops
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FIELDS = list(ops.FIELDS)
SIZES = (8, 12, 80)      # below one wave row; not a multiple of 16; a masked tail past 64 (80 * 80 = 100 * 64)


@pytest.fixture(scope="module")
def gold():
    return load_golden("datasets.npz")


@pytest.fixture(scope="module")
def data(gold):
    return {f: torch.from_numpy(gold[f"data_{f}"]) for f in FIELDS}


_cache = {}


def fields_of(n, T=ops.GOLDEN_T, time_last=False):
    """Seeded CPU fields, drawn once per size and left unchanged."""
    key = (n, T, time_last)
    if key not in _cache:
        _cache[key] = ops.make_data(ops.GOLDEN_N, T, n, seed=n, time_last=time_last)
    return _cache[key]


def same(a, b):
    a = a.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def same_dicts(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert same(got[k], want[k]), k


def batches(n):
    N = ops.GOLDEN_N
    out = [[4], [5, 0, 5]]                                    # batch 1; unsorted with a repeat
    if n == 8:
        out.append([(7 * k + 3) % N for k in range(70)])       # more than a wave of samples
    return out


# ----------------------------------------------------------------------------- windows
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("time_last", [False, True])
@pytest.mark.parametrize("steps,out_steps", ops.WINDOW_CASES)
@pytest.mark.parametrize("n", SIZES)
def test_window_batches_are_bit_equal(n, steps, out_steps, time_last, dtype):
    from torch_cfd_amd.datasets import SpatioTemporalDataset

    d = fields_of(n, time_last=time_last)
    ds = SpatioTemporalDataset(d, n_samples=ops.GOLDEN_N, fields=FIELDS, data_time_last=time_last, steps=steps,
                               out_steps=out_steps, dtype=dtype, device=DEV)
    assert ds.data["vorticity"].dtype == torch.float32 and tuple(ds.data["vorticity"].shape) == tuple(d["vorticity"].shape)
    assert not hasattr(ds, "data_input")
    last = ops.GOLDEN_T - steps - out_steps
    for idx in batches(n):
        starts = [(0, last, last // 2)[k % 3] for k in range(len(idx))]
        if len(idx) == 1:
            starts = [last]
        got = ds.batch(idx, starts)
        want = ops.window_batch(d, idx, starts, steps, out_steps, time_last, dtype)
        for g, w in zip(got, want):
            same_dicts(g, w)
            assert g["time_steps"].dtype == torch.int64
    got = ds.__getitem__(2, 0)
    want = ops.window_item(d, 2, 0, steps, out_steps, time_last, dtype)
    for g, w in zip(got, want):
        same_dicts(g, w)


def test_window_items_equal_every_golden_record(gold, data):
    from torch_cfd_amd.datasets import SpatioTemporalDataset

    seen = 0
    for tl in (False, True):
        d = {f: (v.permute(0, 2, 3, 1).contiguous() if tl else v) for f, v in data.items()}
        for steps, out_steps in ops.WINDOW_CASES:
            for train, ns in ((True, 4), (False, 2)):
                ds = SpatioTemporalDataset(d, n_samples=ns, train=train, fields=FIELDS, data_time_last=tl, steps=steps,
                                           out_steps=out_steps, device=DEV)
                for idx, start in ((0, 0), (ns - 1, ops.GOLDEN_T - steps - out_steps)):
                    tag = f"win_tl{int(tl)}_{steps}_{out_steps}_tr{int(train)}_{idx}_{start}"
                    for side, dd in zip(("inp", "out"), ds.__getitem__(idx, start)):
                        for k, v in dd.items():
                            assert same(v, torch.from_numpy(gold[f"{tag}_{side}_{k}"])), (tag, side, k)
                            seen += 1
    assert seen == 2 * 3 * 2 * 2 * 2 * 3
    ds = SpatioTemporalDataset(data, n_samples=4, fields=FIELDS, steps=3, out_steps=2, dtype=torch.float64, device=DEV)
    assert same(ds.__getitem__(1, 2)[0]["vorticity"], torch.from_numpy(gold["win_f64_inp_vorticity"]))


# ----------------------------------------------------------------------------- FNO3d batches
def _modules(stats, cls):
    """nn.ModuleDict of normalisers carrying the given statistics, through load_state_dict."""
    out = nn.ModuleDict()
    for f, (mean, std) in stats.items():
        out[f] = cls(device=DEV)
        out[f].load_state_dict({"mean": mean, "std": std})
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("out_steps", [5, 10])       # runs of t straddle the 16-byte vectors of the stores
@pytest.mark.parametrize("n", SIZES)
def test_fno3d_batches_are_bit_equal(n, out_steps, dtype):
    from torch_cfd_amd.datasets import SpatioTemporalDatasetFixedTime, UnitGaussianNormalizer

    d = fields_of(n, T=14)
    kw = dict(T_start=1, steps=3, out_steps=out_steps)
    # Identity: the raw fields
    ref = ops.FixedTime(d, n_samples=ops.GOLDEN_N, train=True, inp_stats=False, out_stats=False, dtype=dtype, **kw)
    ds = SpatioTemporalDatasetFixedTime(d, n_samples=ops.GOLDEN_N, train=True, fields=FIELDS, inp_normalizer=False,
                                        out_normalizer=False, dtype=dtype, device=DEV, **kw)
    assert isinstance(ds.inp_normalizer["vorticity"], nn.Identity)
    assert tuple(ds.data_input["stream"].shape) == (ops.GOLDEN_N, 3, n, n) and ds.data_input["stream"].dtype == torch.float32
    assert tuple(ds.data["stream"].shape) == (ops.GOLDEN_N, n, n, out_steps)
    for idx in batches(n):
        got, want = ds.batch(idx), ref.batch(idx)
        for g, w in zip(got, want):
            same_dicts(g, w)
        assert tuple(got[0]["vorticity"].shape) == (len(idx), 6, n, n, out_steps)
    # the coordinate channels are torch.linspace meshes
    inp = ds.batch([1, 3])[0]["stream"].cpu()
    lin_n, lin_t = torch.linspace(0, 1, n, dtype=dtype), torch.linspace(0, 1, out_steps, dtype=dtype)
    assert torch.equal(inp[:, 0], lin_n[None, :, None, None].expand(2, n, n, out_steps))
    assert torch.equal(inp[:, 1], lin_n[None, None, :, None].expand(2, n, n, out_steps))
    assert torch.equal(inp[:, 2], lin_t[None, None, None, :].expand(2, n, n, out_steps))
    for g, w in zip(ds[4], ref.item(4)):
        same_dicts(g, w)
    # the test split under given statistics: transform(align_shapes=True), then the batch
    stats = ops.FixedTime(d, n_samples=4, train=True, **kw)
    ref = ops.FixedTime(d, n_samples=2, train=False, inp_stats=stats.inp_stats, out_stats=stats.out_stats, dtype=dtype, **kw)
    ds = SpatioTemporalDatasetFixedTime(d, n_samples=2, train=False, fields=FIELDS, dtype=dtype, device=DEV,
                                        inp_normalizer=_modules(stats.inp_stats, UnitGaussianNormalizer),
                                        out_normalizer=_modules(stats.out_stats, UnitGaussianNormalizer), **kw)
    for g, w in zip(ds.batch([1, 0, 1]), ref.batch([1, 0, 1])):
        same_dicts(g, w)


def test_odd_plane_takes_the_scalar_stores():
    """n and out_steps odd: a plane is no whole number of 16-byte vectors."""
    from torch_cfd_amd.datasets import SpatioTemporalDatasetFixedTime

    d = ops.make_data(ops.GOLDEN_N, 14, 9, seed=9)
    kw = dict(T_start=0, steps=2, out_steps=5)
    ref = ops.FixedTime(d, n_samples=ops.GOLDEN_N, inp_stats=False, out_stats=False, **kw)
    ds = SpatioTemporalDatasetFixedTime(d, n_samples=ops.GOLDEN_N, fields=FIELDS, inp_normalizer=False, out_normalizer=False,
                                        device=DEV, **kw)
    for g, w in zip(ds.batch([3, 0, 3, 5]), ref.batch([3, 0, 3, 5])):
        same_dicts(g, w)


# ----------------------------------------------------------------------------- fitted statistics
def _check_stats(mean, std, x64, bound, shape, dtype):
    for got, want in ((mean, x64[0]), (std, x64[1])):
        assert got.dtype == dtype and tuple(got.shape) == shape
        err = (got.cpu().double() - want).abs().max().item()
        print(f"statistic error {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("xdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("N", ops.STATS_N)
def test_fitted_statistics(N, xdtype):
    from torch_cfd_amd.datasets import SpatialGaussianNormalizer, UnitGaussianNormalizer

    x = ops.stats_input(N, xdtype)
    x64, xd = x.double(), x.to(DEV)
    big = x64.abs().max().item()
    b32, b64 = 2.0 ** -23 * big, N * 2.0 ** -52 * big
    unit = UnitGaussianNormalizer(device=DEV)
    y = unit.fit_transform(xd)
    _check_stats(unit.mean, unit.std, (x64.mean(0), x64.std(0)), b32, (3, 8, 8), torch.float32)
    assert list(unit.state_dict()) == ["mean", "std"]
    # the transformed data: the affine kernel applied to the module's own statistics, bit for bit
    assert same(y, ops.transform(x, unit.mean.cpu(), unit.std.cpu()))
    spat = SpatialGaussianNormalizer(device=DEV)
    y = spat.fit_transform(xd)
    _check_stats(spat.mean, spat.std, (x64.mean((0, -1)).unsqueeze(-1), x64.std((0, -1)).unsqueeze(-1)),
                 b32 if xdtype == torch.float32 else b64, (3, 8, 1), xdtype)
    assert same(y, ops.transform(x, spat.mean.cpu(), spat.std.cpu()))
    # two runs give the same bits
    for cls, first in ((UnitGaussianNormalizer, unit), (SpatialGaussianNormalizer, spat)):
        again = cls(device=DEV)
        again.fit_transform(xd)
        assert torch.equal(again.mean, first.mean) and torch.equal(again.std, first.std)


@pytest.mark.parametrize("space", [False, True])
def test_fit_on_the_golden_train_split(gold, data, space):
    """The data set fits its own normalisers: statistics within twice the bound of the golden file's, and the statistic shapes
    of normalize_space_only (steps, n, 1) and (n, n, 1)."""
    from torch_cfd_amd.datasets import SpatialGaussianNormalizer, SpatioTemporalDatasetFixedTime, UnitGaussianNormalizer

    ds = SpatioTemporalDatasetFixedTime(data, train=True, fields=FIELDS, inp_normalizer=True, normalize_space_only=space,
                                        out_normalizer=True, device=DEV, **ops.FIXED)
    steps, To, n = ops.FIXED["steps"], ops.FIXED["out_steps"], ops.GOLDEN_n
    shapes = {"inp": (steps, n, 1) if space else (steps, n, n), "out": (n, n, 1) if space else (n, n, To)}
    for f in FIELDS:
        big = data[f].abs().max().item()
        for side, norm in (("inp", ds.inp_normalizer), ("out", ds.out_normalizer)):
            assert type(norm[f]) is (SpatialGaussianNormalizer if space else UnitGaussianNormalizer)
            for k in ("mean", "std"):
                got, want = getattr(norm[f], k), torch.from_numpy(gold[f"fixed_sp{int(space)}_{side}_{k}_{f}"])
                assert got.dtype == want.dtype and tuple(got.shape) == shapes[side] == tuple(want.shape)
                err = (got.cpu().double() - want.double()).abs().max().item()
                print(f"{f} {side} {k}: {err:.3e} (bound {2 * 2.0 ** -23 * big:.3e})")
                assert err <= 2 * 2.0 ** -23 * big
        # the stored fields are the transform of the raw windows under the data set's OWN statistics, bit for bit
        raw = data[f][:4, 1:4]
        assert same(ds.data_input[f], ops.transform(raw, ds.inp_normalizer[f].mean.cpu(), ds.inp_normalizer[f].std.cpu()))


# ----------------------------------------------------------------------------- transforms under the golden statistics
@pytest.mark.parametrize("space", [False, True])
def test_transforms_and_their_gradients(gold, data, space):
    from torch_cfd_amd.datasets import SpatialGaussianNormalizer, UnitGaussianNormalizer

    cls = SpatialGaussianNormalizer if space else UnitGaussianNormalizer
    tag = f"fixed_sp{int(space)}"
    stat = lambda side, k: torch.from_numpy(gold[f"{tag}_{side}_{k}_vorticity"])
    inp, out = cls(device=DEV), cls(device=DEV)
    inp.load_state_dict({"mean": stat("inp", "mean"), "std": stat("inp", "std")})
    out.load_state_dict({"mean": stat("out", "mean"), "std": stat("out", "std")})
    assert inp.mean.is_cuda and list(out.state_dict()) == ["mean", "std"]
    raw = data["vorticity"][:4, 1:4].contiguous()                       # the train split's input window (N, steps, n, n)
    assert same(inp.transform(raw.to(DEV)), torch.from_numpy(gold[f"{tag}_train_input_vorticity"]))
    u = torch.from_numpy(gold[f"{tag}_train_target_vorticity"])[:3].contiguous()
    want = torch.from_numpy(gold[f"{tag}_decode_vorticity"])
    assert same(out.inverse_transform(u.to(DEV)), want) and same(out(u.to(DEV)), want)
    # gradients against autograd through the restatement, under a seeded cotangent
    g = torch.Generator().manual_seed(3)
    for fn, ref_fn, x, (mean, std) in (
            (inp.transform, ops.transform, raw, (stat("inp", "mean"), stat("inp", "std"))),
            (lambda z: inp.transform(z, align_shapes=True), ops.transform_aligned, raw, (stat("inp", "mean"), stat("inp", "std"))),
            (out.inverse_transform, ops.inverse_transform_aligned, u, (stat("out", "mean"), stat("out", "std")))):
        for dt in (torch.float32, torch.float64):
            xc = x.to(dt).requires_grad_(True)
            xd = x.to(dt).to(DEV).requires_grad_(True)
            yc, yd = ref_fn(xc, mean, std), fn(xd)
            assert same(yd.detach(), yc.detach())
            w = torch.randn(yc.shape, generator=g, dtype=torch.float64).to(yc.dtype)
            (gc,) = torch.autograd.grad(yc, xc, w)
            (gd,) = torch.autograd.grad(yd, xd, w.to(DEV))
            assert same(gd, gc)


@pytest.mark.parametrize("space", [False, True])
def test_test_split_under_the_train_modules_matches_golden(gold, data, space):
    from torch_cfd_amd.datasets import SpatialGaussianNormalizer, SpatioTemporalDatasetFixedTime, UnitGaussianNormalizer

    cls = SpatialGaussianNormalizer if space else UnitGaussianNormalizer
    tag = f"fixed_sp{int(space)}"
    stats = {side: {f: tuple(torch.from_numpy(gold[f"{tag}_{side}_{k}_{f}"]) for k in ("mean", "std")) for f in FIELDS}
             for side in ("inp", "out")}
    kw = {**ops.FIXED, "n_samples": 2}
    ds = SpatioTemporalDatasetFixedTime(data, train=False, fields=FIELDS, inp_normalizer=_modules(stats["inp"], cls),
                                        normalize_space_only=space, out_normalizer=_modules(stats["out"], cls), device=DEV, **kw)
    for f in FIELDS:
        assert same(ds.data_input[f], torch.from_numpy(gold[f"{tag}_test_input_{f}"]))
        assert same(ds.data[f], torch.from_numpy(gold[f"{tag}_test_target_{f}"]))
    inp, out = ds[1]
    assert same(inp["vorticity"], torch.from_numpy(gold[f"{tag}_test_item1_inp_vorticity"]))
    assert same(out["vorticity"], torch.from_numpy(gold[f"{tag}_test_item1_out_vorticity"]))


def test_float64_batches_of_float32_fields_match_golden(gold, data):
    from torch_cfd_amd.datasets import SpatioTemporalDatasetFixedTime, UnitGaussianNormalizer

    stats = {side: {f: tuple(torch.from_numpy(gold[f"fixed_sp0_{side}_{k}_{f}"]) for k in ("mean", "std")) for f in FIELDS}
             for side in ("inp", "out")}
    # the train split's rows 0 .. 3 are the last 4 of a "test split" of the first 4 samples: same windows, same statistics
    head = {f: v[:4] for f, v in data.items()}
    ds = SpatioTemporalDatasetFixedTime(head, train=False, fields=FIELDS, dtype=torch.float64, device=DEV,
                                        inp_normalizer=_modules(stats["inp"], UnitGaussianNormalizer),
                                        out_normalizer=_modules(stats["out"], UnitGaussianNormalizer), **ops.FIXED)
    assert same(ds[0][0]["stream"], torch.from_numpy(gold["fixed_f64_item0_inp_stream"]))


def test_add_grid_3d_matches_golden(gold, data):
    from torch_cfd_amd.datasets import add_grid_3d

    for name, (x, kw) in ops.grid3d_cases(data).items():
        got = add_grid_3d(x.to(DEV), **kw)
        assert got.is_cuda and same(got, torch.from_numpy(gold[name])), name


def test_differently_typed_sides_still_batch(data):
    """float64 statistics on the input side, the target left alone: the two stored fields differ in dtype after the
    normalisation and are widened to one; the batch equals the oracle's."""
    from torch_cfd_amd.datasets import SpatialGaussianNormalizer, SpatioTemporalDatasetFixedTime

    kw = {**ops.FIXED, "n_samples": 2}
    train = ops.FixedTime(data, train=True, space_only=True, **ops.FIXED)
    stats = {f: (m.double(), s.double()) for f, (m, s) in train.inp_stats.items()}
    ref = ops.FixedTime(data, train=False, inp_stats=stats, out_stats=False, **kw)
    ds = SpatioTemporalDatasetFixedTime(data, train=False, fields=FIELDS, inp_normalizer=_modules(stats, SpatialGaussianNormalizer),
                                        out_normalizer=False, device=DEV, **kw)
    assert ds.data_input["stream"].dtype == ds.data["stream"].dtype == torch.float64
    for g, w in zip(ds.batch([1, 0]), ref.batch([1, 0])):
        same_dicts(g, w)


# ----------------------------------------------------------------------------- loader and loops
def _collated(batch):
    return [{k: v.cpu() for k, v in side.items()} for side in batch]


@pytest.mark.parametrize("shuffle", [False, True])
def test_batchloader_epoch_equals_dataloader(data, shuffle):
    from torch_cfd_amd.datasets import BatchLoader, SpatioTemporalDataset, SpatioTemporalDatasetFixedTime

    windows = SpatioTemporalDataset(data, n_samples=6, fields=FIELDS, steps=3, out_steps=2, device=DEV)    # random starts
    fixed = SpatioTemporalDatasetFixedTime(data, n_samples=6, fields=FIELDS, inp_normalizer=True, out_normalizer=True,
                                           device=DEV, **{k: v for k, v in ops.FIXED.items() if k != "n_samples"})
    for ds in (windows, fixed):
        np.random.seed(11)
        want = [_collated(b) for b in DataLoader(ds, batch_size=4, shuffle=shuffle, generator=torch.Generator().manual_seed(8))]
        np.random.seed(11)
        got = [_collated(b) for b in BatchLoader(ds, 4, shuffle=shuffle, generator=torch.Generator().manual_seed(8))]
        assert len(got) == len(want) == 2
        for g, w in zip(got, want):
            for gs, ws in zip(g, w):
                same_dicts(gs, ws)


class _Mean(nn.Module):
    """A model of the FNO3d interface, small enough to reason about: a weighted mean of the input steps."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor([0.5, 0.25, 0.125]))

    def forward(self, a):
        return torch.einsum("bcxyt,c->bxyt", a[:, 3:], self.w), None


def test_eval_epoch_ns_is_the_mean_of_the_batch_metrics(data):
    from torch_cfd_amd.datasets import BatchLoader, SpatioTemporalDatasetFixedTime
    from torch_cfd_amd.pipeline import eval_epoch_ns

    ds = SpatioTemporalDatasetFixedTime(data, n_samples=6, fields=FIELDS, inp_normalizer=True, out_normalizer=True, device=DEV,
                                        **{k: v for k, v in ops.FIXED.items() if k != "n_samples"})
    model = _Mean().to(DEV)
    metric = lambda x, y: ((x - y) ** 2).mean().sqrt()
    norm = ds.out_normalizer
    vals = []
    with torch.no_grad():
        for inp, out in BatchLoader(ds, 4):
            pred = norm["vorticity"].inverse_transform(model(inp["vorticity"])[0])
            vals.append(metric(pred, norm["vorticity"].inverse_transform(out["vorticity"])).item())
    want = np.mean(np.asarray(vals), axis=0)
    got = eval_epoch_ns(model, metric, BatchLoader(ds, 4), DEV, normalizer=norm)
    print(f"eval_epoch_ns {got!r} vs {want!r}")
    assert len(vals) == 2 and abs(got - want) <= 1e-12 * abs(want)
    got2, preds, targets = eval_epoch_ns(model, metric, BatchLoader(ds, 4), DEV, normalizer=norm, return_output=True)
    assert got2 == got and tuple(preds.shape) == tuple(targets.shape) == (6, 8, 8, 5) and not preds.is_cuda


def test_train_batch_ns_steps_a_small_fno3d(data):
    from torch_cfd_amd.datasets import BatchLoader, SpatioTemporalDatasetFixedTime
    from torch_cfd_amd.fno import FNO3d
    from torch_cfd_amd.pipeline import train_batch_ns

    ds = SpatioTemporalDatasetFixedTime(data, n_samples=6, fields=FIELDS, inp_normalizer=True, out_normalizer=True, device=DEV,
                                        **{k: v for k, v in ops.FIXED.items() if k != "n_samples"})
    torch.manual_seed(0)
    model = FNO3d(2, 2, 2, 4, input_channel=ops.FIXED["steps"], num_spectral_layers=2).to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    loss_fn = lambda x, y: ((x - y).flatten(1).norm(dim=1) / y.flatten(1).norm(dim=1)).mean()
    batch = next(iter(BatchLoader(ds, 4)))
    loss = train_batch_ns(model, loss_fn, batch, opt, DEV, grad_clip=1.0, normalizer=ds.out_normalizer)
    assert loss.dim() == 0 and torch.isfinite(loss).item()
    changed = [not torch.equal(b, p.detach()) for b, p in zip(before, model.parameters())]
    assert all(changed), changed
