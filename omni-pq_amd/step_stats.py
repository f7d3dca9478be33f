"""The reference's stat_dict loop (train.py:578-606) without its per-step host reads:

    stat_dict['grad_norm'] = grad_total_norm
    for key in end_points:
        if 'loss' in key or 'acc' in key or 'ratio' in key:
            stat_dict[key] += end_points[key] if isinstance(end_points[key], float) else end_points[key].item()
    ... every print_freq steps: log stat_dict[key] / print_freq, then zero it

`.item()` on about a hundred device scalars per step stops the host from running ahead of the GPU a hundred times.
`StepStats` keeps the window on the device instead: one launch per step (include/omnipq_optim.h: omnipq_stats_accumulate, one
thread per key) adds every selected scalar into an f64 slot of its own -- the sequential float64 sum in step order, the bits
of the reference's Python-float `+=` -- and `read()` brings the whole window back with ONE copy per print_freq steps.

    stats = StepStats()
    stats.accumulate(objective.stats, optimizer)        # per step; captured: CapturedStep(..., stats=lambda: objective.stats)
    if (batch_idx + 1) % print_freq == 0:
        window = stats.read()                           # {name: sum}, .steps, .last; window.means(print_freq)

The launch is capturable: under a captured graph the sources' addresses are fixed, the table is built once; eagerly the
scalars are new tensors every step and the 16-byte records are re-uploaded when an address has changed.
"""
import ctypes
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "pointnet2")):
    if _p not in sys.path:
        sys.path.append(_p)

ENTRY = np.dtype([("src", "<u8"), ("kind", "<i4"), ("mode", "<i4")])        # include/omnipq_optim.h: 16 bytes
MAX_ENTRIES = 4096
_KIND = {torch.float32: 0, torch.float64: 1}
SUM, LAST = 0, 1
GRAD_NORM = "grad_norm"


def _ext():
    import pointnet2_utils
    return pointnet2_utils._load_ext()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _selected(key):
    return "loss" in key or "acc" in key or "ratio" in key          # train.py:581


class Window(dict):
    """{name: sum over the window} as read() returns it; `steps` applying steps were accumulated, `calls` launches seen,
    `last[name]` is each key's most recent value (`grad_norm` is a last value in both)."""

    def __init__(self, sums, last, steps, calls, last_mode=()):
        super().__init__(sums)
        self.last, self.steps, self.calls = last, steps, calls
        self._last_mode = frozenset(last_mode)

    def means(self, divisor=None):
        """sum / divisor per key: the steps accumulated, or the caller's print_freq as the reference divides (train.py:591).
        Last-value keys (grad_norm) are passed through, as the reference logs them."""
        d = self.steps if divisor is None else divisor
        if not d:
            raise ZeroDivisionError("Window.means: no step was accumulated")
        return {k: (v if k in self._last_mode else v / d) for k, v in self.items()}


class StepStats:
    def __init__(self):
        self.names = None            # keys of the device table, in order
        self.constants = {}          # key -> Python float added per accumulated step at read time
        self._modes = None
        self._key = None             # (address, dtype) per entry of the table on the device
        self.entries = self.sums = self.last = self.window = None
        self._buf = self._pinned = None          # sums, last and window are views into ONE device buffer: one copy, one memset
        self.device = None
        self.table_uploads = 0       # how often the 16-byte records were sent to the device
        self.copies = 0              # device-to-host copies issued by read()
        self._pending = None         # the sources of a captured call, until retarget() writes their addresses into the table
        self._held = None            # the scalars the table points at: they stay allocated while it does

    # ---- train.py:581's rule -------------------------------------------------------------------------------------------------
    @staticmethod
    def select(mapping):
        """-> ({key: 0-dim floating device tensor}, {key: Python float}) of the keys the reference accumulates: those
        containing 'loss', 'acc' or 'ratio'.  A Python float (the reference's `0.0` placeholders) is kept as a host constant;
        a tensor that is not a scalar, or not floating point, is not a statistic and is left out, like every other key."""
        tensors, constants = {}, {}
        for key, v in mapping.items():
            if not isinstance(key, str) or not _selected(key):
                continue
            if isinstance(v, float):
                constants[key] = v
            elif torch.is_tensor(v) and v.dim() == 0 and v.dtype in _KIND:
                tensors[key] = v
        return tensors, constants

    # ---- the device table ------------------------------------------------------------------------------------------------------
    def _build(self, sources, modes):
        names = list(sources)
        n = len(names)
        if not 1 <= n <= MAX_ENTRIES:
            raise ValueError(f"StepStats: {n} selected scalars; the launch takes between 1 and {MAX_ENTRIES}")
        dev = sources[names[0]].device
        for k in names:
            t = sources[k]
            if t.device != dev or t.dim() != 0 or t.dtype not in _KIND:
                raise ValueError(f"StepStats: `{k}` must be a 0-dim float32 / float64 tensor on {dev}")
        if dev.type != "cuda":
            raise RuntimeError("CPU not supported")          # like the native ops: no CPU path in the product
        key = tuple((sources[k].data_ptr(), sources[k].dtype) for k in names)
        if self.names is not None and names != self.names:
            raise RuntimeError("StepStats: the selected keys changed inside a window (read() first): "
                               f"{sorted(set(names) ^ set(self.names))}")
        if self.names is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("StepStats: the first accumulate() of a table allocates its device and pinned buffers, which a "
                                   "stream capture cannot do -- call it once eagerly first (CapturedStep's warm-up steps do)")
            self.names, self._modes, self.device = names, [modes[k] for k in names], dev
            self.entries = torch.zeros(n * ENTRY.itemsize, dtype=torch.uint8, device=dev)
            self._buf = torch.zeros(2 * n + 2, dtype=torch.float64, device=dev)
            self.sums, self.last = self._buf[:n], self._buf[n:2 * n]
            self.window = self._buf[2 * n:].view(torch.int64)
            self._pinned = torch.zeros(2 * n + 2, dtype=torch.float64, pin_memory=True)
        if key != self._key:
            if torch.cuda.is_current_stream_capturing():
                # nothing may be uploaded now: the launch is recorded against the table's buffers, retarget() fills them
                self._key = None
                self._pending = dict(sources)
                return
            rec = np.zeros(n, dtype=ENTRY)
            for i, k in enumerate(names):
                rec[i] = (sources[k].data_ptr(), _KIND[sources[k].dtype], self._modes[i])
            self.entries.copy_(torch.from_numpy(rec.view(np.uint8)))
            self._key = key
            self._held = dict(sources)
            self.table_uploads += 1

    def reset(self):
        """The window restarts from zero: one memset launch on the current stream."""
        if self._buf is not None:
            with torch.no_grad():
                self._buf.zero_()

    def retarget(self):
        """After a capture: point the table the captured launch reads at the scalars the capture allocated."""
        if self._pending is not None:
            pending, self._pending = self._pending, None
            self._build(pending, dict(zip(self.names, self._modes)))

    def accumulate(self, mapping, optimizer=None, last=()):
        """One launch on the current stream: every selected scalar of `mapping` is added into its slot; the keys named in
        `last` keep their most recent value instead of a sum (fixed with the first call of a table).  optimizer (an
        optim.FusedAdamW): `grad_norm` joins as a last-value entry reading optimizer.result[0] (train.py:578), and with
        accum_steps > 1 only the applying micro-batch accumulates (the launch reads the optimiser's apply mark, so it must
        follow the optimiser's launches on the stream); the others are counted in `calls` only.
        The set of tensor keys is fixed with a table's first call: a key that is a tensor in one step and a Python float (or
        absent) in another raises "keys changed" -- a criterion that reports a term sometimes as a placeholder and sometimes as
        a tensor should report it as a tensor always (SemiSupervisedObjective.stats does)."""
        tensors, constants = self.select(mapping)
        modes = {k: (LAST if k in last else SUM) for k in tensors}
        accum = None
        if optimizer is not None:
            tensors[GRAD_NORM] = optimizer.grad_total_norm
            modes[GRAD_NORM] = LAST
            accum = optimizer.accum
        self._build(tensors, modes)
        for k, c in constants.items():
            self.constants[k] = c
        ext = _ext()
        ext._run(ext._lib0.omnipq_stats_accumulate, self.sums, len(self.names), _ptr(self.entries), _ptr(self.sums),
                 _ptr(self.last), _ptr(self.window), _ptr(accum))

    # ---- the read-back ---------------------------------------------------------------------------------------------------------
    def read(self, reset=True):
        """-> Window: {name: sum} with .steps, .calls and .last.  ONE device-to-host copy of sums, last and window through one
        pinned buffer (the host waits for it: this is the window's one synchronising read); reset: the window restarts from
        zero with one memset launch on the same stream, outside any graph.  A host constant contributes constant * steps."""
        if self.names is None:
            raise RuntimeError("StepStats.read: nothing was accumulated yet")
        n = len(self.names)
        self._pinned.copy_(self._buf, non_blocking=True)        # (the two counters' bits travel as f64)
        self.copies += 1
        torch.cuda.current_stream(self.device).synchronize()
        host = self._pinned.numpy()
        steps, calls = (int(x) for x in host[2 * n:].view(np.int64))
        sums = {k: float(host[i]) for i, k in enumerate(self.names)}
        last = {k: float(host[n + i]) for i, k in enumerate(self.names)}
        for k, c in self.constants.items():
            s = 0.0
            for _ in range(steps):
                s += c                   # the reference's own repeated `+=`, not a product
            sums[k], last[k] = s, c
        if reset:
            self.reset()
        return Window(sums, last, steps, calls, (k for k, m in zip(self.names, self._modes) if m == LAST))
