"""Mean-teacher weight averaging of the reference's training step (train.py:435-439):

    update_ema_variables(model, ema_model, alpha, global_step)

Same name, arguments and arithmetic as the reference's function; on the GPU every parameter of the pair is
updated by ONE launch (`omnipq_ema_update`, 3 x 71 MB of HBM traffic for PQ-Transformer's 17.9 M parameters)
instead of two elementwise launches per parameter tensor (~620).  The device-side table of (ema, param, numel)
is built once per model pair and follows in-place parameter updates (addresses do not change); replaced
parameters rebuild it.

alpha is an ARGUMENT of that launch, so it cannot be part of a captured step.  Where the optimiser is
`optim.FusedAdamW`, `attach_teacher(model, ema_model, alpha)` (`train_step.CapturedStep(ema_in_step=True)`)
runs the same arithmetic inside the optimiser's own update launch, with alpha formed on the device from a
step count that lives there: the same bits, no launch and no host call per step.
"""
import os
import sys
import weakref

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "pointnet2")):
    if _p not in sys.path:
        sys.path.append(_p)

_TABLES = weakref.WeakKeyDictionary()          # ema_model -> (key, table, chunks, keepalive)


def ema_alpha(alpha, global_step):
    """Use the true average until the exponential average is more correct (train.py:436-437)."""
    return min(1.0 - 1.0 / (global_step + 1), alpha)


def _table(model, ema_model):
    pairs = [(e, p) for e, p in zip(ema_model.parameters(), model.parameters())]
    key = tuple((e.data_ptr(), p.data_ptr(), e.numel()) for e, p in pairs)
    hit = _TABLES.get(ema_model)
    if hit is not None and hit[0] == key:
        return hit
    rec = np.dtype([("ema", "<u8"), ("param", "<u8"), ("numel", "<i8")])
    tab = np.zeros(len(pairs), dtype=rec)
    chunks = []
    for i, (e, p) in enumerate(pairs):
        if e.dtype != torch.float32 or p.dtype != torch.float32 or not e.is_contiguous() or not p.is_contiguous() \
                or e.shape != p.shape:
            return None
        tab[i] = (e.data_ptr(), p.data_ptr(), e.numel())
        chunks += [(i, c) for c in range((e.numel() + 4095) // 4096)]
    dev = pairs[0][0].device
    hit = (key, torch.from_numpy(tab.view(np.uint8).copy()).to(dev),
           torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev), len(pairs))
    _TABLES[ema_model] = hit
    return hit


def update_ema_variables(model, ema_model, alpha, global_step):
    a = ema_alpha(alpha, global_step)
    first = next(ema_model.parameters(), None)
    if first is None:
        return a
    if not first.is_cuda:
        raise RuntimeError("CPU not supported")      # like the native ops: no CPU path in the product
    hit = _table(model, ema_model)
    if hit is None:
        raise RuntimeError("update_ema_variables: parameters must be contiguous float32 tensors of equal shapes")
    import sa_fused
    _, table, chunks, nseg = hit
    sa_fused._call(sa_fused._lib.omnipq_ema_update, table, nseg, int(chunks.shape[0]), sa_fused._p(table),
                   sa_fused._p(chunks), a, 1.0 - a)
    return a
