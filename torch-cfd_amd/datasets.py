"""Device-resident data sets, Gaussian normalisers and one-launch batches for the FNO training loops.

Drop-in for ``fno/datasets.py`` of the reference (``UnitGaussianNormalizer`` :21-104, ``SpatialGaussianNormalizer`` :107-121,
``add_grid_3d`` :124-162, ``SpatioTemporalDataset`` :373-453, ``SpatioTemporalDatasetFixedTime`` :456-564); the ``.mat`` data
set ``NavierStokesDataset`` is not here.  The reference builds every sample on the CPU in ``Dataset.__getitem__``, stacks
the samples in the collate step and ships the batch with ``.to(device)``.  Here the fields of the ``.pt`` dict that
``data_gen.generate_*_dataset`` writes stay on the HIP device as stored, and

* ``batch(indices)`` of either data set is ONE kernel launch per field (``tcfd_data_window``, ``tcfd_data_fno3d_batch``,
  csrc/tcfd_data.hip): the permuted clone ``data_input`` of the reference and the repeated ``(3 + steps, n, n, out_steps)``
  FNO3d input are never held for more than the batch;
* the normalisers fit on ``tcfd_data_moments`` (fp64 accumulation in a fixed order) and transform on ``tcfd_data_affine``,
  differentiable with respect to ``x`` -- ``pipeline.train_batch_ns`` decodes the model output before the loss;
* ``BatchLoader`` iterates ``dataset.batch`` in the order ``torch.utils.data.DataLoader`` (no workers) would visit the
  samples, random window starts included.

Every class takes ``device="cuda"`` and a path or an already loaded dict.  HIP only: the kernels raise ``TcfdError`` for a
CPU tensor.  The module imports, and ``BatchLoader.plan()`` runs, without a GPU.
"""
from __future__ import annotations

import ctypes
from os import PathLike
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

__all__ = ["UnitGaussianNormalizer", "SpatialGaussianNormalizer", "add_grid_3d", "SpatioTemporalDataset",
           "SpatioTemporalDatasetFixedTime", "BatchLoader"]


# ----------------------------------------------------------------------------- kernel calls
def _code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return _lib.TCFD_C64
    if dtype == torch.float64:
        return _lib.TCFD_C128
    raise TypeError(f"float32 or float64 data only, got {dtype}")


def _need_hip(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.TcfdError(f"{what}: expected a HIP device tensor (torch-cfd_amd has no CPU fallback), got {t.device}")


def _library():
    """The loaded library; the tcfd_data_* entries were added without a new ABI revision, so a library built before them
    passes the revision check of ``_lib.load`` and is caught here."""
    lib = _lib.load()
    if not hasattr(lib, "tcfd_data_window"):
        raise _lib.TcfdError(f"{_lib.LIB_PATH} was built before the tcfd_data_* entry points existed: rebuild it with "
                             "torch_cfd_amd._lib.build_library(force=True)")
    return lib


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _hip_window(src: torch.Tensor, lists: torch.Tensor, steps: int, out_steps: int, time_last: bool,
                dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """src (N, T, *mesh) or (N, *mesh, T); lists (2, count) int64 on the device (rows, starts) -> the two windows
    (count, *mesh, steps) and (count, *mesh, out_steps) in ``dtype``."""
    _need_hip(src, "tcfd_data_window")
    assert src.is_contiguous() and lists.is_contiguous() and lists.dtype == torch.int64
    count = lists.shape[1]
    mesh = tuple(src.shape[1:-1] if time_last else src.shape[2:])
    total = src.shape[-1] if time_last else src.shape[1]
    points = int(np.prod(mesh, dtype=np.int64))
    a = torch.empty((count, *mesh, steps), dtype=dtype, device=src.device)
    b = torch.empty((count, *mesh, out_steps), dtype=dtype, device=src.device)
    with torch.cuda.device(src.device):
        rc = _library().tcfd_data_window(src.data_ptr(), a.data_ptr(), b.data_ptr(), lists[0].data_ptr(), lists[1].data_ptr(),
                                          count, src.shape[0], total, points, steps, out_steps, int(time_last), _code(src.dtype),
                                          _code(dtype), _stream(src.device))
    _lib.check(rc, "tcfd_data_window")
    return a, b


def _hip_fno3d_batch(field: torch.Tensor, target: torch.Tensor, rows: torch.Tensor, grids: Sequence[torch.Tensor],
                     dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """field (N, steps, n, n), target (N, n, n, To), rows (count,) int64 on the device -> (count, 3 + steps, n, n, To) and
    (count, n, n, To) in ``dtype``."""
    _need_hip(field, "tcfd_data_fno3d_batch")
    N, steps, n, n2 = field.shape
    To = target.shape[-1]
    if n != n2 or tuple(target.shape) != (N, n, n, To) or field.dtype != target.dtype:
        raise ValueError(f"field {tuple(field.shape)} {field.dtype} and target {tuple(target.shape)} {target.dtype} do not match")
    assert field.is_contiguous() and target.is_contiguous() and rows.is_contiguous() and rows.dtype == torch.int64
    count = rows.numel()
    inp = torch.empty((count, 3 + steps, n, n, To), dtype=dtype, device=field.device)
    out = torch.empty((count, n, n, To), dtype=dtype, device=field.device)
    gx, gy, gt = grids
    with torch.cuda.device(field.device):
        rc = _library().tcfd_data_fno3d_batch(field.data_ptr(), target.data_ptr(), rows.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                                               gt.data_ptr(), inp.data_ptr(), out.data_ptr(), count, N, steps, n, To,
                                               _code(field.dtype), _code(dtype), _stream(field.device))
    _lib.check(rc, "tcfd_data_fno3d_batch")
    return inp, out


def _hip_affine(x: torch.Tensor, mean: Optional[torch.Tensor], std: torch.Tensor, eps: float, mode: int, inner: int,
                out_dtype: torch.dtype) -> torch.Tensor:
    _need_hip(x, "tcfd_data_affine")
    x = x.contiguous()
    std = std.contiguous()
    mean = None if mean is None else mean.contiguous()
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = _library().tcfd_data_affine(x.data_ptr(), None if mean is None else mean.data_ptr(), std.data_ptr(), out.data_ptr(),
                                          x.numel(), std.numel(), inner, float(eps), mode, _code(x.dtype), _code(std.dtype),
                                          _code(out_dtype), _stream(x.device))
    _lib.check(rc, "tcfd_data_affine")
    return out


def _hip_moments(x: torch.Tensor, spatial: bool, stat_dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mean and unbiased std over axis 0 (shape ``x.shape[1:]``) or, ``spatial``, over axis 0 and the last axis (shape
    ``x.shape[1:-1] + (1,)``)."""
    _need_hip(x, "tcfd_data_moments")
    if x.dim() < 2:
        raise ValueError(f"statistics of a {x.dim()}-d tensor: expected (N, ...)")
    x = x.contiguous()
    rows = x.shape[0]
    inner = x.shape[-1] if spatial else 1
    shape = (*x.shape[1:-1], 1) if spatial else tuple(x.shape[1:])
    count = x.numel() // (rows * inner)
    mean = torch.empty(shape, dtype=stat_dtype, device=x.device)
    std = torch.empty(shape, dtype=stat_dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = _library().tcfd_data_moments(x.data_ptr(), mean.data_ptr(), std.data_ptr(), rows, count, inner, _code(x.dtype),
                                           _code(stat_dtype), _stream(x.device))
    _lib.check(rc, "tcfd_data_moments")
    return mean, std


def _broadcast_plan(x_shape, stat_shape) -> Optional[int]:
    """``inner`` of the kernel's statistic index ``(e / inner) % m`` for ``x (op) stat`` under torch broadcasting, or None
    where the broadcast is not one of the two the modules produce."""
    xs, ss = tuple(x_shape), tuple(stat_shape)
    k = len(ss)
    if k == 0 or len(xs) < k:
        return None
    if xs[len(xs) - k:] == ss:
        return 1
    if ss[-1] == 1 and xs[len(xs) - k:-1] == ss[:-1]:
        return xs[-1]
    return None


class _AffineFn(torch.autograd.Function):
    """mode 0: (x - mean) / (std + eps);  mode 1: x * (std + eps) + mean.  The derivative with respect to x is the same
    kernel on the cotangent with mean = 0."""

    @staticmethod
    def forward(ctx, x, mean, std, eps, mode, inner):
        ctx.save_for_backward(std)
        ctx.cfg = (eps, mode, inner, x.dtype)
        return _hip_affine(x, mean, std, eps, mode, inner, torch.promote_types(x.dtype, std.dtype))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (std,) = ctx.saved_tensors
        eps, mode, inner, x_dtype = ctx.cfg
        return _hip_affine(g, None, std, eps, mode, inner, x_dtype), None, None, None, None, None


def _affine(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, eps: float, mode: int) -> torch.Tensor:
    _need_hip(x, "normalizer")
    mean, std = mean.to(x.device), std.to(x.device)
    inner = _broadcast_plan(x.shape, mean.shape) if mean.shape == std.shape else None
    if inner is None:
        raise _lib.TcfdError(f"normalizer: statistics of shape {tuple(mean.shape)} do not broadcast over the trailing axes of "
                             f"{tuple(x.shape)} the way the fitted module does")
    return _AffineFn.apply(x, mean, std, eps, mode, inner)


# ----------------------------------------------------------------------------- normalisers
class UnitGaussianNormalizer(nn.Module):
    """Point-wise Gaussian normaliser: ``mean`` and unbiased ``std`` over axis 0, stored in float32 whatever the data dtype
    (fno/datasets.py:21-104).  Methods, buffers and ``state_dict`` keys as the reference; ``load_state_dict`` also works on a
    module that was never fitted (the buffers are created from the state)."""

    _spatial = False

    def __init__(self, eps=1e-7, data: Optional[torch.Tensor] = None, device="cuda"):
        super().__init__()
        self.eps = eps
        self.device = device
        if data is not None:
            self._fit_transform(torch.as_tensor(data))

    def _stat_dtype(self, x: torch.Tensor) -> torch.dtype:
        return torch.float32

    def _fit_transform(self, x: torch.Tensor):
        _need_hip(x, type(self).__name__ + ".fit_transform")
        mean, std = _hip_moments(x, self._spatial, self._stat_dtype(x))
        for name, value in (("mean", mean), ("std", std)):
            if name in self._buffers:
                self._buffers[name] = value
            else:
                self.register_buffer(name, value)
        return _affine(x, mean, std, self.eps, 0)

    def fit_transform(self, *args, **kwargs):
        return self._fit_transform(*args, **kwargs)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for name in ("mean", "std"):
            value = state_dict.get(prefix + name)
            if value is not None and name not in self._buffers:
                self.register_buffer(name, torch.empty(value.shape, dtype=value.dtype, device=self.device))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _transform(self, x: torch.Tensor, align_shapes=False, **kwargs):
        if not hasattr(self, "mean"):     # never fitted: mean 0, std 1, as the reference
            _need_hip(x, type(self).__name__ + ".transform")
            return (x - 0) / (1 + self.eps)
        mean, std = self.mean.to(x.device), self.std.to(x.device)
        if align_shapes:
            mean, std = self._align_shapes(x, mean, std, **kwargs)
        return _affine(x, mean, std, self.eps, 0)

    def transform(self, *args, **kwargs):
        return self._transform(*args, **kwargs)

    def inverse_transform(self, x: torch.Tensor, sample_idx=None, align_shapes=True, **kwargs):
        _need_hip(x, type(self).__name__ + ".inverse_transform")
        mean, std, eps = self.mean.to(x.device), self.std.to(x.device), self.eps
        per_sample = tuple(x.shape[1:])
        if align_shapes and (tuple(mean.shape) != per_sample or 1 in per_sample):
            # another resolution, or unit axes that the alignment squeezes away: the reference adds eps BEFORE it resamples
            mean, std = self._align_shapes(x, mean, std + eps, **kwargs)
            eps = 0.0
        if sample_idx is not None:
            # statistics of picked points (composed device ops): the index applies to the leading axis of the buffers when
            # they have the rank of one index tensor, to their second axis when they have one axis more (time first)
            rank = sample_idx[0].dim()
            scale = std + eps
            if self.mean.dim() == rank:
                mean, scale = self.mean[sample_idx], self.std[sample_idx] + self.eps
            elif self.mean.dim() > rank:
                mean, scale = self.mean[:, sample_idx], self.std[:, sample_idx] + self.eps
            return x * scale + mean
        return _affine(x, mean, std, eps, 1)

    def forward(self, *args, **kwargs):
        return self.inverse_transform(*args, **kwargs)

    @staticmethod
    def _align_shapes(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, **kwargs):
        """Statistics for a batch ``x`` whose per-sample shape ``x.shape[1:]`` differs from theirs (another resolution, or the
        unit axis of the spatial normaliser): both are resampled to it by ``F.interpolate`` -- nearest unless ``mode=`` says
        otherwise -- as device torch ops.  Unit axes are squeezed away in either case, which is what the reference returns."""
        per_sample = tuple(x.shape[1:])

        def resample(t):
            return F.interpolate(t.reshape(1, 1, *t.shape), size=per_sample, **kwargs)

        if tuple(mean.shape) != per_sample:
            mean, std = resample(mean), resample(std)
        return mean.squeeze(), std.squeeze()


class SpatialGaussianNormalizer(UnitGaussianNormalizer):
    """Statistics over axis 0 and the LAST axis of whatever it is given, in the data dtype, with a trailing axis of 1
    (fno/datasets.py:107-121).  The reference's docstring assumes (N, n, n, T); the data set hands its time-first input window
    (N, steps, n, n) to it all the same, which gives statistics of shape (steps, n, 1).  That is kept."""

    _spatial = True

    def __init__(self, eps=1e-7, device="cuda"):
        super().__init__(eps=eps, device=device)

    def _stat_dtype(self, x: torch.Tensor) -> torch.dtype:
        return x.dtype


def add_grid_3d(data: torch.Tensor, dim_concat=-1, expand_dim=False, device=None, dtype=torch.float) -> torch.Tensor:
    """The coordinate channels x, y, t (``linspace(0, 1)`` along n, n and T = ``data.shape[3]``) in front of the channels of
    ``data`` along ``dim_concat`` (fno/datasets.py:124-162): (N, n, n, T, C) -> (N, n, n, T, 3 + C); with ``expand_dim`` a
    four-axis (N, n, n, T) gets a new axis at ``dim_concat`` first, along which it is repeated T times, so (N, n, n, C) ->
    (N, n, n, C, 3 + C) and, with ``dim_concat=1``, (N, n, n, T) -> (N, 3 + T, n, n, T).  Device torch ops on the whole tensor;
    the data sets below never call it (their batches come from one kernel)."""
    _need_hip(data, "add_grid_3d")
    device = data.device if device is None else device
    N, n, T = data.shape[0], data.shape[1], data.shape[3]
    if expand_dim:
        data = data.unsqueeze(dim_concat)
        copies = list(data.shape)
        copies[dim_concat] = T
        data = data.expand(copies)
    coords = torch.empty((3, n, n, T), device=device, dtype=dtype)
    along = torch.linspace(0, 1, n, device=device, dtype=dtype)
    coords[0] = along[:, None, None]
    coords[1] = along[None, :, None]
    coords[2] = torch.linspace(0, 1, T, device=device, dtype=dtype)
    if dim_concat == -1:
        coords = coords.movedim(0, -1)
    return torch.cat((coords.expand(N, *coords.shape), data), dim=dim_concat)


# ----------------------------------------------------------------------------- data sets
def _load_fields(data_path, fields) -> Dict[str, torch.Tensor]:
    data = data_path if isinstance(data_path, dict) else torch.load(data_path, map_location="cpu")
    missing = [f for f in fields if f not in data]
    if missing:
        raise KeyError(f"fields {missing} not in the data ({sorted(data.keys())})")
    return {f: data[f] for f in fields}


def _index_list(indices, length: int) -> List[int]:
    if isinstance(indices, torch.Tensor):
        indices = indices.tolist()
    if isinstance(indices, (int, np.integer)):
        indices = [indices]
    out = []
    for i in indices:
        i = int(i)
        if not -length <= i < length:
            raise IndexError(f"sample {i} outside a data set of {length}")
        out.append(i % length)
    return out


class SpatioTemporalDataset(torch.utils.data.Dataset):
    """Windows ``[s, s + steps)`` -> ``[s + steps, s + steps + out_steps)`` of trajectories (fno/datasets.py:373-453).

    The fields stay on the device as stored -- (N, T, n, n), or (N, n, n, T) with ``data_time_last`` -- in the file's dtype.
    ``__getitem__`` returns the reference's ``(inp, out)`` dicts (time last, cast to ``dtype``, int64 ``time_steps`` on the
    host); ``batch(indices, start_steps=None)`` returns the same for a list of samples, stacked, from one launch per field.
    ``total_steps`` is ``size(1)`` of the stored field, as in the reference (with ``data_time_last`` that is n, not T)."""

    def __init__(self, data_path: Union[PathLike, str, dict], n_samples: int = 1024, train=True,
                 fields=["vorticity", "stream"], data_time_last: bool = False, steps=10, out_steps=None, T_start=None,
                 dtype=torch.float32, device="cuda"):
        self.data_path = data_path
        self.n_samples = n_samples
        self.train = train
        self.fields = list(fields)
        self.steps = steps
        self.out_steps = out_steps if out_steps is not None else steps
        self.T_start = T_start
        self.data_time_last = data_time_last
        self.dtype = dtype
        self.device = torch.device(device)
        self._initialize()

    def __len__(self):
        return self.n_samples

    def _initialize(self):
        data = _load_fields(self.data_path, self.fields)
        first = data[self.fields[0]]
        self.total_steps = first.size(1)
        self.time_len = first.size(-1) if self.data_time_last else first.size(1)
        pick = slice(0, self.n_samples) if self.train else slice(-self.n_samples, None)
        self.data = {f: v[pick].to(self.device).contiguous() for f, v in data.items()}
        have = self.data[self.fields[0]].size(0)
        if have != self.n_samples:
            raise ValueError(f"n_samples = {self.n_samples}, the data hold {have}")

    def draw_start(self) -> int:
        """The start ``__getitem__`` uses when none is given: ``T_start``, else one ``np.random.randint`` draw."""
        if self.T_start is None:
            return int(np.random.randint(0, self.total_steps - (self.out_steps + self.steps + 1)))
        return self.T_start

    def _lists(self, indices, start_steps) -> Tuple[List[int], List[int]]:
        rows = _index_list(indices, self.n_samples)
        if start_steps is None:
            starts = [self.draw_start() for _ in rows]
        elif isinstance(start_steps, (int, np.integer)):
            starts = [int(start_steps)] * len(rows)
        else:
            starts = [int(s) for s in start_steps]
        if len(starts) != len(rows):
            raise ValueError(f"{len(rows)} samples, {len(starts)} starts")
        for s in starts:
            if s < 0 or s + self.steps + self.out_steps > self.time_len:
                raise ValueError(f"window [{s}, {s + self.steps + self.out_steps}) outside the {self.time_len} recorded steps")
        return rows, starts

    def batch(self, indices, start_steps=None):
        rows, starts = self._lists(indices, start_steps)
        if self.device.type != "cuda":
            raise _lib.TcfdError(f"SpatioTemporalDataset.batch: HIP devices only (no CPU fallback), the data are on {self.device}")
        lists = torch.tensor([rows, starts], dtype=torch.int64).to(self.device)
        inp, out = dict(), dict()
        for f in self.fields:
            inp[f], out[f] = _hip_window(self.data[f], lists, self.steps, self.out_steps, self.data_time_last, self.dtype)
        s = torch.tensor(starts, dtype=torch.int64)[:, None]
        inp["time_steps"] = s + torch.arange(self.steps)
        out["time_steps"] = s + self.steps + torch.arange(self.out_steps)
        return inp, out

    def __getitem__(self, idx, start_steps=None):
        inp, out = self.batch([idx], None if start_steps is None else [start_steps])
        return {k: v[0] for k, v in inp.items()}, {k: v[0] for k, v in out.items()}


class SpatioTemporalDatasetFixedTime(SpatioTemporalDataset):
    """The FNO3d data set (fno/datasets.py:456-564): one fixed window per trajectory, normalised, and the input repeated
    along the output steps behind the three coordinate channels.

    Sliced once; ``inp_normalizer`` / ``out_normalizer`` are ``True`` (fit, train split), an ``nn.ModuleDict`` (applied with
    ``transform(align_shapes=True)`` on the test split) or ``False`` (``nn.Identity``).  Kept on the device: the normalised
    input ``data_input[f]`` (N, steps, n, n) and target ``data[f]`` (N, n, n, out_steps).  ``__getitem__`` returns
    ``(3 + steps, n, n, out_steps)`` and ``(n, n, out_steps)``; ``batch(indices)`` writes ``(b, 3 + steps, n, n, out_steps)``
    and ``(b, n, n, out_steps)`` in one launch per field, so the repeated tensor exists for the batch alone."""

    def __init__(self, data_path: Union[PathLike, str, dict], n_samples: int = 1024, train=True,
                 fields=["vorticity", "stream"], data_time_last: bool = False, T_start=0, steps=10, out_steps=10,
                 inp_normalizer: Union[bool, nn.ModuleDict] = None, normalize_space_only: bool = False, out_normalizer=True,
                 dtype=torch.float32, device="cuda"):
        super().__init__(data_path=data_path, n_samples=n_samples, train=train, fields=fields, data_time_last=data_time_last,
                         T_start=T_start, steps=steps, out_steps=out_steps, dtype=dtype, device=device)
        if self.device.type != "cuda":
            raise _lib.TcfdError(f"SpatioTemporalDatasetFixedTime: HIP devices only (no CPU fallback), got {self.device}")
        self.inp_normalizer = inp_normalizer
        self.normalize_space_only = normalize_space_only
        self.out_normalizer = out_normalizer
        self._slicing_in_time()
        self._normalize()
        self._add_grid()

    def _slicing_in_time(self):
        """``data_input[f]`` (N, steps, n, n) and ``data[f]`` (N, n, n, out_steps), both in the file's dtype, from one window
        launch per field; the full trajectories are dropped."""
        rows, starts = self._lists(range(self.n_samples), self.T_start)
        lists = torch.tensor([rows, starts], dtype=torch.int64).to(self.device)
        self.data_input = dict()
        for f in self.fields:
            full = self.data[f]
            window, self.data[f] = _hip_window(full, lists, self.steps, self.out_steps, self.data_time_last, full.dtype)
            self.data_input[f] = window.permute(0, 3, 1, 2).contiguous()

    def normalize(self, data, normalizer):
        """``(data, modules)``: ``False`` leaves the fields alone under ``nn.Identity`` modules; ``True`` on the train split
        fits one normaliser per field and stores the transformed field; an ``nn.ModuleDict`` on the test split applies its
        modules with aligned shapes.  Anything else (``None``, modules handed to a train split) changes nothing."""
        missing = [f for f in self.fields if f not in data]
        if missing:
            raise KeyError(f"fields {missing} not in the data")
        if normalizer is False:
            return data, nn.ModuleDict({f: nn.Identity() for f in self.fields})
        if normalizer is True and self.train:
            kind = SpatialGaussianNormalizer if self.normalize_space_only else UnitGaussianNormalizer
            fitted = nn.ModuleDict({f: kind(device=self.device) for f in self.fields})
            for f, module in fitted.items():
                data[f] = module.fit_transform(data[f])
            return data, fitted
        if isinstance(normalizer, nn.ModuleDict) and not self.train:
            for f in self.fields:
                data[f] = normalizer[f].transform(data[f], align_shapes=True)
        return data, normalizer

    def _normalize(self):
        self.data_input, self.inp_normalizer = self.normalize(self.data_input, self.inp_normalizer)
        self.data, self.out_normalizer = self.normalize(self.data, self.out_normalizer)
        # differently typed statistics on the two sides (or one side left alone) can leave the two fields in different
        # dtypes; the batch kernel reads one source dtype, and widening the narrower one is exact
        for f in self.fields:
            wide = torch.promote_types(self.data_input[f].dtype, self.data[f].dtype)
            self.data_input[f], self.data[f] = self.data_input[f].to(wide), self.data[f].to(wide)

    def _add_grid(self):
        """The three coordinate tables of the (3, n, n, T) positional encoding, in ``dtype``."""
        n, n2, n_t = self.data[self.fields[0]].shape[1:]
        if n != n2:
            raise ValueError(f"square meshes only, got {n} x {n2}")
        lin = lambda k: torch.linspace(0, 1, k, dtype=self.dtype)   # on the host, as the reference; then uploaded
        self._tables = tuple(lin(k).to(self.device) for k in (n, n, n_t))

    @property
    def grid(self) -> torch.Tensor:
        """(3, n, n, T) coordinate meshes (the reference's attribute; assembled on request, the kernel reads the tables)."""
        return torch.stack(torch.meshgrid(*self._tables, indexing="ij"))

    def batch(self, indices, start_steps=None):
        rows = torch.tensor(_index_list(indices, self.n_samples), dtype=torch.int64).to(self.device)
        inp, out = dict(), dict()
        for f in self.fields:
            inp[f], out[f] = _hip_fno3d_batch(self.data_input[f], self.data[f], rows, self._tables, self.dtype)
        return inp, out

    def __getitem__(self, idx):
        inp, out = self.batch([idx])
        return {k: v[0] for k, v in inp.items()}, {k: v[0] for k, v in out.items()}


# ----------------------------------------------------------------------------- loader
class BatchLoader:
    """Iterates ``dataset.batch(indices[, starts])`` in the order ``torch.utils.data.DataLoader(dataset, batch_size, shuffle,
    drop_last=drop_last, generator=generator)`` with no workers visits the samples.

    That loader draws one int64 base seed from the generator when an iterator is made, BEFORE its sampler's ``randperm``
    (and the sampler seeds a generator of its own from the global one when none is given); after the last index the
    sampler draws one more ``randperm`` for its empty tail.  All of it is restated, so equally seeded generators give equal
    epochs, one after the other.  Random window starts come from ``dataset.draw_start()``, once per sample in batch order."""

    def __init__(self, dataset, batch_size: int = 1, shuffle: bool = False, drop_last: bool = False, generator=None):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.drop_last = drop_last
        self.generator = generator

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def plan(self) -> List[Tuple[List[int], Optional[List[int]]]]:
        """One epoch's ``(indices, starts)`` per batch (``starts`` is None for a data set without ``draw_start``).  Consumes
        the generators exactly as one pass over the DataLoader would; touches no device."""
        n = len(self.dataset)
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)          # the loader's base seed
        if self.shuffle:
            gen = self.generator
            if gen is None:
                gen = torch.Generator()
                gen.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            order = torch.randperm(n, generator=gen).tolist()
            torch.randperm(n, generator=gen)                                          # the sampler's empty tail
        else:
            order = list(range(n))
        draw = getattr(self.dataset, "draw_start", None)
        out = []
        for i in range(0, n, self.batch_size):
            indices = order[i:i + self.batch_size]
            if len(indices) < self.batch_size and self.drop_last:
                break
            out.append((indices, [draw() for _ in indices] if draw is not None else None))
        return out

    def __iter__(self):
        for indices, starts in self.plan():
            yield self.dataset.batch(indices) if starts is None else self.dataset.batch(indices, starts)
