#!/usr/bin/env python
"""Generate tests/golden/datasets.npz by IMPORTING THE REFERENCE's fno/datasets.py (CPU only, deterministic).

Run only where a checkout of the reference is present (read-only), naming it:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_datasets.py /path/to/reference

fno/datasets.py imports two third-party packages that need not be installed, so stand-ins of this script's own are
registered first: an empty ``h5py`` (only the ``.mat`` data set would call it) and a ``tensordict`` whose ``TensorDict`` is a
dict subclass with what the data sets use -- row slicing, ``clone`` and item assignment.  fno/pipeline.py is NOT imported
(it needs tensorboard).  The records carry the names tests/datasets_ops.py::golden_records gives them; every tensor comes
from the reference's classes: ``SpatioTemporalDataset.__getitem__``, ``SpatioTemporalDatasetFixedTime`` with its fitted
``UnitGaussianNormalizer`` / ``SpatialGaussianNormalizer`` modules, ``inverse_transform`` and ``add_grid_3d``.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


class TensorDict(dict):
    def __init__(self, data=None, batch_size=None, **kw):
        super().__init__(data or {})
        self.batch_size = batch_size

    def __getitem__(self, key):
        if isinstance(key, str):
            return dict.__getitem__(self, key)
        return TensorDict({k: v[key] for k, v in self.items()})

    def clone(self):
        return TensorDict({k: v.clone() for k, v in self.items()}, self.batch_size)


def import_reference(path):
    sys.modules["h5py"] = types.ModuleType("h5py")
    td = types.ModuleType("tensordict")
    td.TensorDict = TensorDict
    sys.modules["tensordict"] = td
    sys.path.insert(0, path)
    from fno import datasets
    return datasets


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    import datasets_ops as ops

    N, T, n = ops.GOLDEN_N, ops.GOLDEN_T, ops.GOLDEN_n
    data = ops.make_data(N, T, n)
    store = {f"data_{f}": v.numpy() for f, v in data.items()}
    record = ops.np_record(store)
    fields = list(ops.FIELDS)
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for tl in (False, True):
            paths[tl] = os.path.join(tmp, f"data_tl{int(tl)}.pt")
            torch.save({f: (v.permute(0, 2, 3, 1).contiguous() if tl else v) for f, v in data.items()}, paths[tl])
        for tl in (False, True):
            for steps, out_steps in ops.WINDOW_CASES:
                for train, ns in ((True, 4), (False, 2)):
                    ds = ref.SpatioTemporalDataset(paths[tl], n_samples=ns, train=train, fields=fields, data_time_last=tl,
                                                   steps=steps, out_steps=out_steps)
                    for idx, start in ((0, 0), (ns - 1, T - steps - out_steps)):
                        inp, out = ds.__getitem__(idx, start)
                        tag = f"win_tl{int(tl)}_{steps}_{out_steps}_tr{int(train)}_{idx}_{start}"
                        for side, dd in (("inp", inp), ("out", out)):
                            for k, v in dd.items():
                                record(f"{tag}_{side}_{k}", v)
        ds = ref.SpatioTemporalDataset(paths[False], n_samples=4, train=True, fields=fields, steps=3, out_steps=2,
                                       dtype=torch.float64)
        record("win_f64_inp_vorticity", ds.__getitem__(1, 2)[0]["vorticity"])
        fixed = dict(ops.FIXED)
        for space in (False, True):
            tag = f"fixed_sp{int(space)}"
            tr = ref.SpatioTemporalDatasetFixedTime(paths[False], train=True, fields=fields, inp_normalizer=True,
                                                    normalize_space_only=space, out_normalizer=True, **fixed)
            te = ref.SpatioTemporalDatasetFixedTime(paths[False], train=False, fields=fields, inp_normalizer=tr.inp_normalizer,
                                                    normalize_space_only=space, out_normalizer=tr.out_normalizer,
                                                    **{**fixed, "n_samples": 2})
            for f in fields:
                for side, norm in (("inp", tr.inp_normalizer), ("out", tr.out_normalizer)):
                    sd = norm[f].state_dict()
                    assert sorted(sd) == ["mean", "std"], sorted(sd)
                    record(f"{tag}_{side}_mean_{f}", sd["mean"])
                    record(f"{tag}_{side}_std_{f}", sd["std"])
                record(f"{tag}_train_input_{f}", tr.data_input[f])
                record(f"{tag}_train_target_{f}", tr.data[f])
                record(f"{tag}_test_input_{f}", te.data_input[f])
                record(f"{tag}_test_target_{f}", te.data[f])
            for name, dset, idx in (("train", tr, 2), ("test", te, 1)):
                inp, out = dset[idx]
                record(f"{tag}_{name}_item{idx}_inp_vorticity", inp["vorticity"])
                record(f"{tag}_{name}_item{idx}_out_vorticity", out["vorticity"])
            u = tr.data["vorticity"][:3]
            record(f"{tag}_decode_vorticity", tr.out_normalizer["vorticity"].inverse_transform(u))
        d64 = ref.SpatioTemporalDatasetFixedTime(paths[False], train=True, fields=fields, inp_normalizer=True, out_normalizer=True,
                                                 dtype=torch.float64, **fixed)
        record("fixed_f64_item0_inp_stream", d64[0][0]["stream"])
    for name, (x, kw) in ops.grid3d_cases(data).items():
        record(name, ref.add_grid_3d(x, **kw))
    dst = os.path.join(HERE, "datasets.npz")
    np.savez_compressed(dst, **store)
    print(f"wrote {dst}: {len(store)} records, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
