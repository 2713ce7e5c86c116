"""Plain-torch restatement (CPU, no kernels) of the reference's data sets and normalisers: the oracle of
tests/test_datasets_gpu.py at sizes the golden file does not hold.  tests/test_datasets_host.py shows that it reproduces
every record of tests/golden/datasets.npz -- which the REFERENCE's own classes wrote -- bit for bit; that licenses it.

The memory layouts follow the reference step by step (a permuted view, its clone, a slice of that, another permuted view):
the order in which torch sums a reduction depends on the strides, and the fitted statistics are compared bit for bit.
"""
import numpy as np
import torch
import torch.nn.functional as F

FIELDS = ("vorticity", "stream")
EPS = 1e-7

# the golden cases: N samples of T steps on an n x n mesh
GOLDEN_N, GOLDEN_T, GOLDEN_n = 6, 9, 8
WINDOW_CASES = ((3, 2), (1, 1), (4, 5))          # (steps, out_steps) with T = 9
FIXED = dict(n_samples=4, T_start=1, steps=3, out_steps=5)


def make_data(N, T, n, seed=0, dtype=torch.float32, time_last=False):
    """Seeded fields (N, T, n, n) -- or (N, n, n, T) -- of ``randn + 0.5`` (the stream function scaled down)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, f in enumerate(FIELDS):
        x = (torch.randn(N, T, n, n, generator=g, dtype=torch.float64) + 0.5) * (1.0 if k == 0 else 0.125)
        x = x.to(dtype)
        out[f] = x.permute(0, 2, 3, 1).contiguous() if time_last else x
    return out


def stats_input(N, dtype=torch.float32):
    """The (N, 3, 8, 8) ``randn + 0.5`` input of the fitted-statistics checks, N in STATS_N."""
    g = torch.Generator().manual_seed(N)
    return (torch.randn(N, 3, 8, 8, generator=g, dtype=torch.float64) + 0.5).to(dtype)


STATS_N = (5, 37, 1000)


# ----------------------------------------------------------------------------- coordinate channels
def add_grid_3d(x, dim_concat=-1, expand_dim=False, dtype=torch.float32):
    """x, y, t coordinate channels in front of the channels of x along ``dim_concat``; with ``expand_dim`` x first gets that
    axis, T = x.shape[3] copies long."""
    N, n, T = x.shape[0], x.shape[1], x.shape[3]
    if expand_dim:
        x = torch.stack([x] * T, dim=dim_concat)
    ax, at = torch.linspace(0, 1, n, dtype=dtype), torch.linspace(0, 1, T, dtype=dtype)
    chans = [ax[:, None, None].expand(n, n, T), ax[None, :, None].expand(n, n, T), at[None, None, :].expand(n, n, T)]
    grid = torch.stack(chans, dim=-1 if dim_concat == -1 else 0)
    return torch.cat((grid[None].expand(N, *grid.shape), x), dim=dim_concat)


def grid3d_cases(data):
    """name -> (input, keyword arguments) of the add_grid_3d records."""
    five = torch.stack([data[f][:2].permute(0, 2, 3, 1) for f in FIELDS], dim=-1)          # (N, n, n, T, 2)
    four = data["vorticity"][:2].permute(0, 2, 3, 1)
    return {"grid3d_cat_last": (five, {}),
            "grid3d_expand_last": (four[..., :3], dict(expand_dim=True)),
            "grid3d_expand_first": (four[..., :5], dict(dim_concat=1, expand_dim=True)),
            "grid3d_expand_first_f64": (four[..., :5], dict(dim_concat=1, expand_dim=True, dtype=torch.float64))}


# ----------------------------------------------------------------------------- normalisers
def unit_fit(x):
    """mean and unbiased std over axis 0, stored in float32."""
    return torch.as_tensor(x.mean(0), dtype=torch.float32), torch.as_tensor(x.std(0), dtype=torch.float32)


def spatial_fit(x):
    """over axis 0 and the last axis, in the data dtype, trailing axis of 1."""
    return x.mean((0, -1)).unsqueeze(-1), x.std((0, -1)).unsqueeze(-1)


def transform(x, mean, std, eps=EPS):
    return (x - mean) / (std + eps)


def inverse_transform(x, mean, std, eps=EPS):
    return (x * (std + eps)) + mean


def align(x, mean, std, **kw):
    """Statistics brought to the trailing shape of x (nearest interpolation unless ``mode`` is given), then squeezed."""
    size = list(x.shape[1:])
    if len(size) != mean.ndim or any(s != m for s, m in zip(size, mean.shape)):
        mean = F.interpolate(mean[None, None, ...], size=size, **kw)
        std = F.interpolate(std[None, None, ...], size=size, **kw)
    return mean.squeeze(), std.squeeze()


def transform_aligned(x, mean, std, eps=EPS):
    m, s = align(x, mean, std)
    return (x - m) / (s + eps)


def inverse_transform_aligned(x, mean, std, eps=EPS):
    m, s = align(x, mean, std + eps)
    return (x * s) + m


# ----------------------------------------------------------------------------- data sets
def split(data, n_samples, train):
    return {f: (v[:n_samples] if train else v[-n_samples:]) for f, v in data.items()}


def time_last_views(data, data_time_last):
    """The (N, n, n, T) fields the reference indexes: a permuted VIEW of time-first storage."""
    return {f: (v if data_time_last else v.permute(0, 2, 3, 1)) for f, v in data.items()}


def window_item(data, idx, start, steps, out_steps, data_time_last=False, dtype=torch.float32):
    """(inp, out) of SpatioTemporalDataset.__getitem__(idx, start) over the already split ``data``."""
    views = time_last_views(data, data_time_last)
    inp, out = {}, {}
    for f, v in views.items():
        inp[f] = v[idx, ..., start:start + steps].to(dtype)
        out[f] = v[idx, ..., start + steps:start + steps + out_steps].to(dtype)
    inp["time_steps"] = torch.arange(start, start + steps)
    out["time_steps"] = torch.arange(start + steps, start + steps + out_steps)
    return inp, out


def window_batch(data, indices, starts, steps, out_steps, data_time_last=False, dtype=torch.float32):
    items = [window_item(data, i, s, steps, out_steps, data_time_last, dtype) for i, s in zip(indices, starts)]
    return tuple({k: torch.stack([it[side][k] for it in items]) for k in items[0][side]} for side in (0, 1))


class FixedTime:
    """SpatioTemporalDatasetFixedTime restated.  ``inp_stats`` / ``out_stats``: None fits (train split), a dict
    ``{field: (mean, std)}`` applies it with aligned shapes (test split), False leaves the data alone."""

    def __init__(self, data, n_samples, train=True, data_time_last=False, T_start=0, steps=10, out_steps=10, inp_stats=None,
                 space_only=False, out_stats=None, dtype=torch.float32):
        self.dtype, self.out_steps, self.space_only = dtype, out_steps, space_only
        views = time_last_views(split(data, n_samples, train), data_time_last)
        clones = {f: v.clone() for f, v in views.items()}
        self.data_input, self.data = {}, {}
        for f in views:
            self.data_input[f] = clones[f][..., T_start:T_start + steps].permute(0, 3, 1, 2)      # (N, steps, n, n)
            self.data[f] = views[f][..., T_start + steps:T_start + steps + out_steps]             # (N, n, n, out_steps)
        self.data_input, self.inp_stats = self._normalize(self.data_input, inp_stats)
        self.data, self.out_stats = self._normalize(self.data, out_stats)
        n, _, n_t = next(iter(self.data.values())).shape[1:]
        lin = lambda k: torch.linspace(0, 1, k, dtype=dtype)
        self.grid = torch.stack(torch.meshgrid(lin(n), lin(n), lin(n_t), indexing="ij"))

    def _normalize(self, data, stats):
        if stats is None:
            stats = {}
            for f, x in data.items():
                stats[f] = spatial_fit(x) if self.space_only else unit_fit(x)
                data[f] = transform(x, *stats[f])
        elif stats is not False:
            for f, x in data.items():
                data[f] = transform_aligned(x, *stats[f])
        return data, stats

    def item(self, idx):
        inp, out = {}, {}
        for f in self.data:
            x = self.data_input[f][idx]
            rep = [1] * (x.ndim + 1)
            rep[-1] = self.out_steps
            inp[f] = torch.cat((self.grid, x.unsqueeze(-1).repeat(rep))).to(self.dtype)
            out[f] = self.data[f][idx].to(self.dtype)
        return inp, out

    def batch(self, indices):
        items = [self.item(i) for i in indices]
        return tuple({k: torch.stack([it[side][k] for it in items]) for k in items[0][side]} for side in (0, 1))


# ----------------------------------------------------------------------------- the golden records, by name
def golden_records(data, record):
    """Calls ``record(name, tensor)`` for every record of tests/golden/datasets.npz, computed by THIS module from the
    golden file's own fields ``data`` (time first).  tests/golden/make_golden_datasets.py writes the same names from the
    reference's classes."""
    N = GOLDEN_N
    for tl in (False, True):
        d = {f: (v.permute(0, 2, 3, 1).contiguous() if tl else v) for f, v in data.items()}
        for steps, out_steps in WINDOW_CASES:
            for train, ns in ((True, 4), (False, 2)):
                part = split(d, ns, train)
                for idx, start in ((0, 0), (ns - 1, GOLDEN_T - steps - out_steps)):
                    inp, out = window_item(part, idx, start, steps, out_steps, tl)
                    tag = f"win_tl{int(tl)}_{steps}_{out_steps}_tr{int(train)}_{idx}_{start}"
                    for side, dd in (("inp", inp), ("out", out)):
                        for k, v in dd.items():
                            record(f"{tag}_{side}_{k}", v)
    inp64, _ = window_item(split(data, 4, True), 1, 2, 3, 2, False, torch.float64)
    record("win_f64_inp_vorticity", inp64["vorticity"])
    for space in (False, True):
        tag = f"fixed_sp{int(space)}"
        tr = FixedTime(data, train=True, space_only=space, **FIXED)
        te = FixedTime(data, n_samples=2, train=False, space_only=space, inp_stats=tr.inp_stats, out_stats=tr.out_stats,
                       **{k: v for k, v in FIXED.items() if k != "n_samples"})
        for f in FIELDS:
            for side, stats in (("inp", tr.inp_stats), ("out", tr.out_stats)):
                record(f"{tag}_{side}_mean_{f}", stats[f][0])
                record(f"{tag}_{side}_std_{f}", stats[f][1])
            record(f"{tag}_train_input_{f}", tr.data_input[f])
            record(f"{tag}_train_target_{f}", tr.data[f])
            record(f"{tag}_test_input_{f}", te.data_input[f])
            record(f"{tag}_test_target_{f}", te.data[f])
        for name, ds, idx in (("train", tr, 2), ("test", te, 1)):
            inp, out = ds.item(idx)
            record(f"{tag}_{name}_item{idx}_inp_vorticity", inp["vorticity"])
            record(f"{tag}_{name}_item{idx}_out_vorticity", out["vorticity"])
        # the decode of train_batch_ns: inverse_transform (aligned shapes) of a batch of targets
        u = tr.data["vorticity"][:3]
        record(f"{tag}_decode_vorticity", inverse_transform_aligned(u, *tr.out_stats["vorticity"]))
    d64 = FixedTime(data, train=True, dtype=torch.float64, **FIXED)
    record("fixed_f64_item0_inp_stream", d64.item(0)[0]["stream"])
    for name, (x, kw) in grid3d_cases(data).items():
        record(name, add_grid_3d(x, **kw))


def np_record(store):
    def record(name, t):
        store[name] = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return record
