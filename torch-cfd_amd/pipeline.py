"""The batch loops of the FNO notebooks: ``train_batch_ns`` and ``eval_epoch_ns`` with the signatures of the reference's
``fno/pipeline.py`` (:38-103), without its tensorboard / tqdm imports and its directory creation at import.

Differences that do not change a result:

* a batch from ``datasets.BatchLoader`` is on the device already, so moving it there is a no-op;
* a model that returns a tuple -- ``FNO3d`` returns ``(prediction, None)`` -- is unpacked (the reference hands the tuple to
  the loss, which fails);
* ``eval_epoch_ns`` passes ``out_steps`` to the model only when one is given (``FNO3d.forward`` takes none), accumulates
  the per-batch metric on the device in float64 and synchronises ONCE, where the reference calls ``.item()`` per batch.
"""
from __future__ import annotations

import numpy as np
import torch

__all__ = ["train_batch_ns", "eval_epoch_ns"]


def _predict(model, data, device, fname, normalizer, **model_kwargs):
    """``(prediction, target)`` of one ``(inp, out)`` batch of dicts, both decoded by ``normalizer[fname]`` when one is given."""
    inp, out = data[0], data[1]
    pred = model(inp[fname].to(device), **model_kwargs)
    if isinstance(pred, (tuple, list)):
        pred = pred[0]
    target = out[fname].to(device)
    if normalizer is None:
        return pred, target
    decode = normalizer[fname].inverse_transform
    return decode(pred), decode(target)


def train_batch_ns(model, loss_func, data, optimizer, device, grad_clip=0, fname="vorticity", normalizer=None):
    """One optimiser step on the batch ``data = (inp, out)`` of dicts; returns the loss tensor."""
    optimizer.zero_grad()
    loss = loss_func(*_predict(model, data, device, fname, normalizer))
    loss.backward()
    if grad_clip > 0:
        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
    optimizer.step()
    return loss


def eval_epoch_ns(model, metric_func, valid_loader, device, fname="vorticity", out_steps=None, normalizer=None,
                  return_output=False):
    """Mean of the per-batch metric over ``valid_loader`` (and, with ``return_output``, the predictions and targets on the
    host)."""
    model.eval()
    model_kwargs = {} if out_steps is None else {"out_steps": out_steps}
    total, count, kept = None, 0, ([], [])
    with torch.no_grad():
        for data in valid_loader:
            pred, target = _predict(model, data, device, fname, normalizer, **model_kwargs)
            if return_output:
                kept[0].append(pred.cpu())
                kept[1].append(target.cpu())
            value = metric_func(pred, target).detach().to(torch.float64)
            total = value if total is None else total + value
            count += 1
    if count == 0:
        raise ValueError("eval_epoch_ns: the loader yielded no batch")
    metric = np.float64((total / count).cpu().numpy())     # the one synchronisation
    if return_output:
        return metric, torch.cat(kept[0]), torch.cat(kept[1])
    return metric
