"""The three lines of the reference's training step that change the weights (train.py:562-566), as this project's own HIP:

    grad_total_norm = clip_grad_norm_(model.parameters(), config.clip_norm)
    optimizer.step()                      # AdamW over two parameter groups (train.py:364-374)

`FusedAdamW` takes torch.optim.AdamW's arguments plus `max_norm` (the clip, fused in), `grad_scale` (the inverse of a
static fp16 loss scale) and `loss_scaler` (a dynamic one, below).  One step is three launches over a device table of all
parameter tensors (include/omnipq_optim.h: squared-norm partials, finalise, update) instead of several dozen multi-tensor
launches driven from the host.  Learning rates, betas, eps, weight decay, max_norm, grad_scale, the step count and the bias
corrections all live in device memory: no launch takes one as an argument, so the launches can be captured into `train_step.CapturedStep`'s graph and a replay
follows whatever an LR scheduler wrote into `param_groups` (`sync_hyperparameters()` stages the rows).

What differs from torch.optim.AdamW, all of it stated rather than hidden:
  * ONE step counter for the whole optimiser (device memory).  `state[p]['step']` is materialised from it by
    `state_dict()`; a loaded state whose parameters disagree on `step` is refused.
  * a step whose gradient norm is not finite changes nothing and counts as `skipped` (torch.amp.GradScaler's rule);
  * `.grad` is read-only: the clipped gradient is never written back (nothing in the reference reads it afterwards);
  * `exp_avg` / `exp_avg_sq` of all parameters are two flat f32 buffers, `state[p]` holds views into them.
`state_dict()` / `load_state_dict()` are interchangeable with torch.optim.AdamW's in both directions.

Gradient accumulation (the reference's `step_freq`: train.py:493-494 zeroes the gradients on the first of k micro-batches,
train.py:562-576 clips and steps on the last): `FusedAdamW(..., accum_steps=k)`.  `step()` / `launch()` are then called once
per MICRO-batch; each call is the same three launches (the omnipq_adamw_accum_* family), which add the gradients into a flat
f32 accumulator laid out like `exp_avg`, and every k-th call clips and applies the SUM -- the reference does not divide its
loss by step_freq either; `grad_scale = 1 / k` gives the mean.  The micro-batch counter is a device word the launches read, so
one captured graph serves every micro-batch; `micro` / `is_update_step` mirror it on the host without reading the device.

Mean-teacher weight averaging (the reference's update_ema_variables, train.py:435-439 and :576): `attach_teacher(model,
ema_model, decay)` makes every applying step average the teacher inside the finalise and update launches -- still three
launches, 8 more bytes per parameter instead of a fourth launch of 12.  alpha = min(1 - 1/(global_step + 1), decay) is formed
on the device from a step count that lives there, so a captured launch averages with the alpha of its own step; the teacher
holds the bits `ema.update_ema_variables` would have left after the step.

Dynamic fp16 loss scaling (torch.amp.GradScaler's other half -- the skip on a non-finite norm is the first):
`FusedAdamW(..., loss_scaler=LossScaler(init_scale, growth_factor, backoff_factor, growth_interval))`.  The scale S and its
growth tracker are GradScaler's two tensors, in device memory; `opt.loss_scale` IS S (a 0-dim f32 view), the caller writes
`(loss * opt.loss_scale).backward(); opt.step()`.  The finalise launch (omnipq_adamw_scaled_finalize, the superset of the other
three) divides the norm and the update's coefficient by the S it reads -- the effective factor is grad_scale / S, the
squared-norm and update launches are unchanged -- and every applying call ends with the recurrence of
torch._amp_update_scale_: a non-finite norm backs S off, `growth_interval` finite ones in a row grow it.  S is constant
over an accumulation window.  A host-side GradScaler cannot do this inside a captured step: its step()/update() read
found_inf on the host.  `scaler_state_dict()` / `load_scaler_state_dict()` speak GradScaler.state_dict()'s keys and types.
"""
import ctypes
import math
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(_HERE, "pointnet2")):
    if _p not in sys.path:
        sys.path.append(_p)

RECORD = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"),
                   ("group", "<i4"), ("reserved", "<i4")])          # include/omnipq_optim.h: 48 bytes
EMA_ONLY = np.dtype([("ema", "<u8"), ("param", "<u8"), ("numel", "<i8")])      # include/omnipq_optim.h: 24 bytes
ROW = 8                  # doubles per hyper-parameter row, floats per coefficient row
CHUNK = 4096             # elements per workgroup (a multiple of 1024); tools/bench_optimizer.py --chunks measures others
_STAGES = 4              # pinned staging rows in rotation: a row is rewritten only after its own copy has completed


def _ext():
    import pointnet2_utils
    return pointnet2_utils._load_ext()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _is_int(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def _is_real(x):
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))


class LossScaler:
    """The configuration of a dynamic loss scale: torch.amp.GradScaler's arguments with torch's defaults.  `init_scale` is where
    FusedAdamW starts; the three others may be changed on the optimiser's copy (`opt.loss_scaler`) at any time and are staged
    by sync_hyperparameters() like a learning rate."""
    __slots__ = ("init_scale", "growth_factor", "backoff_factor", "growth_interval")

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.init_scale, self.growth_factor, self.backoff_factor = init_scale, growth_factor, backoff_factor
        self.growth_interval = growth_interval
        self.validate()
        self.init_scale, self.growth_factor = float(init_scale), float(growth_factor)
        self.backoff_factor, self.growth_interval = float(backoff_factor), int(growth_interval)

    def validate(self):
        if not _is_real(self.init_scale) or not math.isfinite(self.init_scale) or not self.init_scale > 0:
            raise ValueError(f"LossScaler: init_scale must be a finite number > 0, not {self.init_scale!r}")
        with np.errstate(over="ignore", under="ignore"):
            as_f32 = float(np.float32(self.init_scale))
        if as_f32 == 0.0 or not math.isfinite(as_f32):
            raise ValueError(f"LossScaler: init_scale={self.init_scale!r} is zero or infinite in float32, the scale's type")
        if not _is_real(self.growth_factor) or not math.isfinite(self.growth_factor) or not self.growth_factor > 1:
            raise ValueError(f"LossScaler: growth_factor must be a finite number > 1, not {self.growth_factor!r}")
        if not _is_real(self.backoff_factor) or not 0 < self.backoff_factor < 1:
            raise ValueError(f"LossScaler: backoff_factor must be in (0, 1), not {self.backoff_factor!r}")
        if not _is_int(self.growth_interval) or self.growth_interval < 1 or self.growth_interval > 2 ** 31 - 1:
            raise ValueError(f"LossScaler: growth_interval must be an integer in [1, 2^31), not {self.growth_interval!r}")

    def __repr__(self):
        return (f"LossScaler(init_scale={self.init_scale!r}, growth_factor={self.growth_factor!r}, "
                f"backoff_factor={self.backoff_factor!r}, growth_interval={self.growth_interval!r})")


class _Table:
    """The device tables of one (parameter, gradient) address set."""
    __slots__ = ("key", "shape_key", "records", "chunks", "partials", "nrec", "nchunks",
                 "ema_ptrs", "ema_only", "only_chunks", "n_only", "n_only_chunks")     # the teacher's side (attach_teacher)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_norm=0.0, grad_scale=1.0, chunk_elems=CHUNK, accum_steps=1, loss_scaler=None):
        if amsgrad:
            raise NotImplementedError("FusedAdamW: amsgrad is not implemented (the reference does not use it)")
        if maximize:
            raise NotImplementedError("FusedAdamW: maximize is not implemented (the reference does not use it)")
        if chunk_elems <= 0 or chunk_elems % 1024:
            raise ValueError("FusedAdamW: chunk_elems must be a positive multiple of 1024")
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, (int, np.integer)) or accum_steps < 1:
            raise ValueError("FusedAdamW: accum_steps must be an integer >= 1 (the number of micro-batches summed per step)")
        if loss_scaler is not None:
            if not isinstance(loss_scaler, LossScaler):
                raise ValueError("FusedAdamW: loss_scaler is an optim.LossScaler or None (a torch.amp.GradScaler reads found_inf "
                                 "on the host and cannot run inside a captured step)")
            loss_scaler.validate()
            # the optimiser's own copy: growth_factor, backoff_factor and growth_interval may be changed on it
            loss_scaler = LossScaler(loss_scaler.init_scale, loss_scaler.growth_factor, loss_scaler.backoff_factor,
                                     loss_scaler.growth_interval)
        # torch.optim.AdamW validates the values and knows which keys a param_group of THIS torch carries: its defaults are
        # taken over as they are, so that a state_dict of either optimiser has the other's param_groups keys
        probe = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if torch.is_tensor(lr) or any(torch.is_tensor(b) for b in betas):
            raise ValueError("FusedAdamW: lr and betas are Python numbers (they are staged to the device by sync_hyperparameters)")
        super().__init__(params, dict(probe.defaults))
        self.max_norm, self.grad_scale = float(max_norm), float(grad_scale)
        self.chunk_elems = int(chunk_elems)
        self.accum_steps = int(accum_steps)
        plist = [p for g in self.param_groups for p in g["params"]]
        if not plist:
            raise ValueError("FusedAdamW: no parameters")
        dev = plist[0].device
        for p in plist:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise ValueError("FusedAdamW: parameters must be contiguous float32 tensors on one device")
        self.device = dev
        # the moments: two flat buffers.  A parameter's segment starts at the parameter's own phase modulo 16 bytes, so that
        # p, m and v of a chunk move as 16-byte vectors together even where p is a view at an odd offset of a joint matrix
        self._offset, total = {}, 0
        for p in plist:
            total += ((p.data_ptr() >> 2) - total) % 4
            self._offset[p] = total
            total += p.numel()
        self.exp_avg = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        # accumulation: the running sum of the gradients, laid out like exp_avg (a record's segment is found through its
        # exp_avg pointer), and {micro-batches summed, apply mark} in device memory.  accum_steps == 1 allocates neither.
        self.acc = self.accum = None
        if self.accum_steps > 1:
            self.acc = torch.zeros(total + 4, dtype=torch.float32, device=dev)
            self.accum = torch.zeros(2, dtype=torch.int64, device=dev)
        self._micro, self._applied = 0, False
        # mean-teacher averaging inside the launches (attach_teacher): nothing is allocated until a teacher is attached
        self._teacher = None
        self.ema_decay = 0.0
        self.ema_state = self.ema_coef = None
        # dynamic loss scaling: one omnipq_loss_scaler { scale, growth_tracker } in device memory, laid out as the loaded
        # library reports it; its three factors travel in one more row of the staged hyper-parameters (_rows)
        self.loss_scaler = loss_scaler
        self.scaler_state = self.loss_scale = self._tracker = None
        if loss_scaler is not None:
            rec = _ext().loss_scaler_struct()
            if (rec.scale.size, rec.growth_tracker.size) != (4, 4) or rec.scale.offset % 4 or rec.growth_tracker.offset % 4:
                raise RuntimeError("FusedAdamW: the loaded library's struct omnipq_loss_scaler is not { float, int32 }")
            self.scaler_state = torch.zeros(ctypes.sizeof(rec), dtype=torch.uint8, device=dev)
            o = rec.scale.offset
            self.loss_scale = self.scaler_state[o:o + 4].view(torch.float32).reshape(())      # a view: S itself
            o = rec.growth_tracker.offset
            self._tracker = self.scaler_state[o:o + 4].view(torch.int32).reshape(())
            self.loss_scale.fill_(loss_scaler.init_scale)
        ngroups = len(self.param_groups)
        nrows = ngroups + 1 + (loss_scaler is not None)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)             # t, skipped
        self.result = torch.zeros(4, dtype=torch.float32, device=dev)             # total_norm, clip_coef, found_nonfinite, g coefficient
        self.grad_total_norm = self.result[0]                                      # what step() returns: rewritten by every step
        self._coef = torch.zeros(ngroups * ROW, dtype=torch.float32, device=dev)
        self._hyper = torch.zeros((nrows, ROW), dtype=torch.float64, device=dev)
        self._stages = [torch.zeros((nrows, ROW), dtype=torch.float64, pin_memory=dev.type == "cuda")
                        for _ in range(_STAGES if dev.type == "cuda" else 1)]
        self._stage_events = [None] * len(self._stages)
        self._stage_next = 0
        self.staging = self._stages[0]          # the rows staged last
        self._sent = None
        self._table_hit = None
        self.table_builds = 0
        self.sync_hyperparameters()

    def add_param_group(self, param_group):
        if hasattr(self, "_offset"):
            raise NotImplementedError("FusedAdamW: parameter groups are fixed at construction (the moments are two flat "
                                      "buffers laid out over them)")
        super().add_param_group(param_group)

    # ---- moments and state ---------------------------------------------------------------------------------------------------
    def _views(self, p):
        o = self._offset[p]
        return self.exp_avg[o:o + p.numel()].view_as(p), self.exp_avg_sq[o:o + p.numel()].view_as(p)

    def _ensure_state(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            m, v = self._views(p)
            st["step"] = torch.tensor(0.0, dtype=torch.get_default_dtype())
            st["exp_avg"], st["exp_avg_sq"] = m, v
        return st

    @property
    def t(self):
        """optimiser steps taken (reads the device)"""
        return int(self.counters[0])

    @property
    def skipped(self):
        """steps skipped because the gradient norm was not finite (reads the device)"""
        return int(self.counters[1])

    @property
    def micro(self):
        """micro-batches summed into the accumulator since the last applying call, in [0, accum_steps): the host's mirror
        of the device word (no device read -- exact, because a skipped non-finite step resets the device word as well)"""
        return self._micro

    @property
    def is_update_step(self):
        """was the last step() / launch() (or replay of a captured launch()) the applying one?  Host-side, no device read."""
        return self._applied

    # ---- the dynamic loss scale ---------------------------------------------------------------------------------------------
    def _need_scaler(self, what):
        if self.loss_scaler is None:
            raise RuntimeError(f"FusedAdamW.{what}: this optimiser was built without loss_scaler=")

    @property
    def scale_value(self):
        """the loss scale the NEXT step's loss is multiplied by (reads the device); None without a loss scaler"""
        return None if self.loss_scaler is None else float(self.loss_scale)

    @property
    def growth_tracker(self):
        """applying steps with a finite norm since the scale last changed (reads the device); None without a loss scaler"""
        return None if self.loss_scaler is None else int(self._tracker)

    def scaler_state_dict(self):
        """torch.amp.GradScaler.state_dict(): the same keys and value types, so either loads what the other wrote.  Not part
        of state_dict(), which stays torch.optim.AdamW's: save the two next to each other."""
        self._need_scaler("scaler_state_dict")
        return {"scale": self.scale_value, "growth_factor": float(self.loss_scaler.growth_factor),
                "backoff_factor": float(self.loss_scaler.backoff_factor),
                "growth_interval": int(self.loss_scaler.growth_interval), "_growth_tracker": self.growth_tracker}

    def load_scaler_state_dict(self, state_dict):
        """What GradScaler.load_state_dict() accepts.  The scale and the tracker are written to the device on the current
        stream, the factors are staged like hyper-parameters: a captured launch sees all of them on its next replay."""
        self._need_scaler("load_scaler_state_dict")
        if len(state_dict) == 0:
            raise RuntimeError("FusedAdamW.load_scaler_state_dict: the state dict is empty (written by a disabled GradScaler?)")
        tracker = state_dict["_growth_tracker"]
        if not _is_int(tracker) or not 0 <= tracker <= 2 ** 31 - 1:
            raise ValueError(f"FusedAdamW.load_scaler_state_dict: _growth_tracker must be an integer >= 0, not {tracker!r}")
        loaded = LossScaler(state_dict["scale"], state_dict["growth_factor"], state_dict["backoff_factor"],
                            state_dict["growth_interval"])
        self.loss_scaler.growth_factor, self.loss_scaler.backoff_factor = loaded.growth_factor, loaded.backoff_factor
        self.loss_scaler.growth_interval = loaded.growth_interval
        with torch.no_grad():
            self.loss_scale.fill_(loaded.init_scale)
            self._tracker.fill_(int(tracker))
        self.sync_hyperparameters()

    def reset_accumulation(self):
        """Discard a partial sum (where the reference's zero_grad does: the start of an epoch).  The device word is set to 0
        on the current stream, the host does not read the device; the next call overwrites the accumulator."""
        if self.accum is not None:
            with torch.no_grad():
                self.accum.zero_()
        self._micro, self._applied = 0, False

    def replayed(self):
        """A captured launch() was replayed once: advance the host mirror as launch() itself does."""
        self._micro = (self._micro + 1) % self.accum_steps
        self._applied = self._micro == 0

    # ---- the mean teacher ------------------------------------------------------------------------------------------------------
    def attach_teacher(self, model, ema_model, decay, global_step=1):
        """From now on every APPLYING step()/launch() also averages `ema_model` towards `model`, inside the finalise and update
        launches (include/omnipq_optim.h: omnipq_adamw_ema_*): the reference's update_ema_variables(model, ema_model, decay,
        global_step) of train.py:435-439 and :576 with the bits of ema.update_ema_variables called after the step, and
        global_step counted on the device -- a captured launch() takes the alpha of its own step on every replay.  The pairs are
        zip(ema_model.parameters(), model.parameters()), as in ema.py; a parameter without a gradient is averaged too, and so
        is every parameter on a step that is skipped for a non-finite gradient norm.  With accum_steps = k only the k-th
        micro-batch averages and counts.  global_step: the value the FIRST averaging uses; 1 is the reference's first
        (train.py increments model.i in front of the call), a resumed run passes its own or calls set_global_step().
        `ema_decay` may be changed at any time, sync_hyperparameters() stages it like max_norm.  Attach before a capture: a
        captured launch keeps the tables and entry points it was recorded with."""
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"FusedAdamW.attach_teacher: decay must be in [0, 1], not {decay!r}")
        if isinstance(global_step, bool) or not isinstance(global_step, (int, np.integer)) or global_step < 0:
            raise ValueError("FusedAdamW.attach_teacher: global_step must be an integer >= 0")
        teacher, student = list(ema_model.parameters()), list(model.parameters())
        if len(teacher) != len(student):
            raise ValueError(f"FusedAdamW.attach_teacher: the teacher has {len(teacher)} parameters, the model {len(student)}")
        for e, p in zip(teacher, student):
            if p not in self._offset:
                raise ValueError("FusedAdamW.attach_teacher: the model has a parameter this optimiser does not own "
                                 f"(shape {tuple(p.shape)})")
            if e.dtype != torch.float32 or not e.is_contiguous() or e.shape != p.shape or e.device != p.device:
                raise ValueError("FusedAdamW.attach_teacher: every teacher parameter must be a contiguous float32 tensor of its "
                                 f"partner's shape on its partner's device (got {e.dtype}, {tuple(e.shape)} on {e.device} for "
                                 f"{tuple(p.shape)} on {p.device})")
        self._teacher = list(zip(teacher, student))
        self.ema_decay = decay
        self.ema_state = torch.full((1,), int(global_step), dtype=torch.int64, device=self.device)
        self.ema_coef = torch.zeros(2, dtype=torch.float32, device=self.device)          # alpha, beta of the last averaging
        self._table_hit = None
        self.sync_hyperparameters()

    def detach_teacher(self):
        """Back to the launches of an optimiser that never had a teacher; the teacher's weights stay as they are."""
        self._teacher = None
        self.ema_decay = 0.0
        self.ema_state = self.ema_coef = None
        self._table_hit = None
        self.sync_hyperparameters()

    @property
    def global_step(self):
        """the global_step the NEXT averaging will use (reads the device); None without a teacher.  It is the model's `i` of the
        reference, not optimiser state: state_dict() does not carry it, a resumed run hands it to attach_teacher() or
        set_global_step()."""
        return None if self.ema_state is None else int(self.ema_state[0])

    def set_global_step(self, i):
        if self.ema_state is None:
            raise RuntimeError("FusedAdamW.set_global_step: no teacher is attached")
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or i < 0:
            raise ValueError("FusedAdamW.set_global_step: an integer >= 0")
        with torch.no_grad():
            self.ema_state.fill_(int(i))

    def state_dict(self):
        """torch.optim.AdamW's state_dict, with or without a teacher: global_step, the decay and the teacher's weights belong
        to the model pair and its training loop, not to the optimiser."""
        t = float(self.t)                          # the one host read of the device counter
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.tensor(t, dtype=torch.get_default_dtype())
        return super().state_dict()

    def load_state_dict(self, state_dict):
        steps = {float(s["step"]) for s in state_dict["state"].values() if "step" in s}
        if len(steps) > 1:
            raise ValueError(f"FusedAdamW.load_state_dict: the parameters disagree on `step` ({sorted(steps)}); this optimiser "
                             "keeps one step count for all of them")
        for s in state_dict["state"].values():
            if s.get("max_exp_avg_sq") is not None:
                raise NotImplementedError("FusedAdamW.load_state_dict: the state was written with amsgrad=True")
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("FusedAdamW.load_state_dict: amsgrad / maximize are not implemented")
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            for g in self.param_groups:
                for p in g["params"]:
                    st = self.state.get(p)
                    if not st:
                        continue
                    m, v = self._views(p)
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    st["exp_avg"], st["exp_avg_sq"] = m, v
            self.counters[0] = int(steps.pop()) if steps else 0
        self.reset_accumulation()                    # the accumulator is not part of a state_dict (nor is torch's .grad)
        self._sent = None
        self.sync_hyperparameters()

    # ---- hyper-parameters ----------------------------------------------------------------------------------------------------
    def _rows(self):
        ng = len(self.param_groups)
        rows = np.zeros((ng + 1 + (self.loss_scaler is not None), ROW), dtype=np.float64)
        for i, g in enumerate(self.param_groups):
            rows[i, :5] = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
        rows[ng, :3] = (self.max_norm, self.grad_scale, float(self.ema_decay))
        if self.loss_scaler is not None:
            # scaler_cfg of omnipq_adamw_scaled_finalize: one row behind the ones the other launches index by ngroups
            self.loss_scaler.validate()
            rows[ng + 1, :3] = (float(self.loss_scaler.growth_factor), float(self.loss_scaler.backoff_factor),
                                float(self.loss_scaler.growth_interval))
        return rows

    def sync_hyperparameters(self):
        """Stage the rows {lr, beta1, beta2, eps, weight_decay} of every param_group, {max_norm, grad_scale, ema_decay} and -- with
        a loss scaler -- {growth_factor, backoff_factor, growth_interval} to the device when a host value has changed since the last call: pinned staging tensor, non-blocking copy on the current stream, no
        host read of the device.  An LR scheduler keeps working on `param_groups`; step() calls this, and so does
        CapturedStep.step() in front of its replay.  -> True when rows were sent."""
        rows = self._rows()
        if self._sent is not None and np.array_equal(rows, self._sent):
            return False
        i = self._stage_next
        self._stage_next = (i + 1) % len(self._stages)
        if self._stage_events[i] is not None:
            self._stage_events[i].synchronize()          # the copy that last read this staging tensor (_STAGES syncs ago)
        stage = self._stages[i]
        stage.copy_(torch.from_numpy(rows))
        self._hyper.copy_(stage, non_blocking=True)
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._stage_events[i] = ev
        self.staging = stage
        self._sent = rows
        return True

    # ---- the device table ----------------------------------------------------------------------------------------------------
    def _active(self):
        return [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"] if p.grad is not None]

    def _host_tables(self, active):
        ext = _ext()
        rec = np.zeros(len(active), dtype=RECORD)
        chunks = []
        for i, (gi, p) in enumerate(active):
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.shape != p.shape \
                    or not p.is_contiguous():
                raise RuntimeError("FusedAdamW: parameters and gradients must be contiguous float32 tensors of equal shapes")
            m, v = self._ensure_state(p)["exp_avg"], self.state[p]["exp_avg_sq"]
            rec[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi, 0)
            chunks += [(i, c) for c in range((p.numel() + self.chunk_elems - 1) // self.chunk_elems)]
        chunks = np.asarray(chunks, dtype=np.int32).reshape(-1, 2)
        rc = ext._lib0.omnipq_adamw_check_table(len(active), rec.ctypes.data_as(ctypes.c_void_p), int(chunks.shape[0]),
                                                chunks.ctypes.data_as(ctypes.c_void_p), len(self.param_groups), self.chunk_elems)
        if rc != 0:
            raise RuntimeError(f"omnipq_adamw_check_table failed: {ext._lib0.omnipq_error_string(rc).decode()} ({rc})")
        return rec, chunks

    def _teacher_key(self):
        return None if self._teacher is None else tuple((e.data_ptr(), p.data_ptr(), e.numel()) for e, p in self._teacher)

    def _host_teacher_tables(self, active):
        """-> (the teacher's pointer per record of `active`, the {ema, param, numel} records of the pairs whose parameter has no
        gradient, their chunk list), validated by the library"""
        ext = _ext()
        partner = {p: e for e, p in self._teacher}
        ptrs = np.asarray([partner[p].data_ptr() for _, p in active], dtype=np.uint64)
        in_table = {p for _, p in active}
        rest = [(e, p) for e, p in self._teacher if p not in in_table]
        only = np.zeros(len(rest), dtype=EMA_ONLY)
        chunks = []
        for i, (e, p) in enumerate(rest):
            only[i] = (e.data_ptr(), p.data_ptr(), e.numel())
            chunks += [(i, c) for c in range((e.numel() + self.chunk_elems - 1) // self.chunk_elems)]
        chunks = np.asarray(chunks, dtype=np.int32).reshape(-1, 2)
        rc = ext._lib0.omnipq_adamw_check_ema_table(len(ptrs), ptrs.ctypes.data_as(ctypes.c_void_p), len(only),
                                                    only.ctypes.data_as(ctypes.c_void_p), int(chunks.shape[0]),
                                                    chunks.ctypes.data_as(ctypes.c_void_p), self.chunk_elems)
        if rc != 0:
            raise RuntimeError(f"omnipq_adamw_check_ema_table failed: {ext._lib0.omnipq_error_string(rc).decode()} ({rc})")
        return ptrs, only, chunks

    def _table(self, capturing=False):
        """The device table, cached and keyed on the (parameter, gradient) addresses (like ema._table).  capturing: nothing may
        be uploaded now -- the launches are recorded against the table buffers of the last eager step, which must cover the same
        parameters, and `retarget()` writes the addresses of the captured gradients into them once the capture has ended."""
        active = self._active()
        # (the teacher's addresses are part of both keys: another teacher is another table, never a re-targeted one)
        tkey = self._teacher_key()
        key = (tuple((p.data_ptr(), p.grad.data_ptr(), p.numel()) for _, p in active), tkey)
        hit = self._table_hit
        if hit is not None and hit.key == key:
            return hit
        shape_key = (tuple((p.data_ptr(), p.numel(), gi) for gi, p in active), tkey)
        if self._micro != 0 and hit is not None and hit.shape_key != shape_key:
            # a parameter that was absent at micro == 0 would add into whatever an earlier step left in its accumulator
            raise RuntimeError(f"FusedAdamW: the set of parameters with gradients changed after {self._micro} of "
                               f"{self.accum_steps} accumulated micro-batches (reset_accumulation() discards the partial sum)")
        if hit is not None and hit.shape_key == shape_key:
            if capturing:
                hit.key = None                       # stale until retarget()
                return hit
            rec, _ = self._host_tables(active)
            hit.records.copy_(torch.from_numpy(rec.view(np.uint8)))      # same buffers: captured launches keep pointing at them
            hit.key = key
            self.table_builds += 1
            return hit
        if capturing:
            raise RuntimeError("FusedAdamW: the parameters with gradients differ from those of the step before the capture")
        rec, chunks = self._host_tables(active)
        hit = _Table()
        hit.key, hit.shape_key = key, shape_key
        hit.nrec, hit.nchunks = len(active), int(chunks.shape[0])
        hit.records = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
        hit.chunks = torch.from_numpy(chunks.copy()).to(self.device)
        hit.partials = torch.zeros(max(hit.nchunks, 1), dtype=torch.float64, device=self.device)
        hit.ema_ptrs = hit.ema_only = hit.only_chunks = None
        hit.n_only = hit.n_only_chunks = 0
        if self._teacher is not None:
            ptrs, only, only_chunks = self._host_teacher_tables(active)
            hit.n_only, hit.n_only_chunks = len(only), int(only_chunks.shape[0])
            hit.ema_ptrs = torch.from_numpy(ptrs.view(np.uint8).copy()).to(self.device)
            if hit.n_only:
                hit.ema_only = torch.from_numpy(only.view(np.uint8).copy()).to(self.device)
                hit.only_chunks = torch.from_numpy(only_chunks.copy()).to(self.device)
        self._table_hit = hit
        self.table_builds += 1
        return hit

    def retarget(self):
        """After a capture: point the table the captured launches read at the gradients the capture allocated."""
        self._table(capturing=False)

    # ---- the step ------------------------------------------------------------------------------------------------------------
    def launch(self):
        """The three launches on the current stream, hyper-parameters as they are on the device (no staging, no host read):
        what CapturedStep records into its graph.  -> the device tensor grad_total_norm.  accum_steps = k > 1: one call per
        micro-batch, the same three launches every time; the k-th call applies the sum, the others only add and count.
        With a loss scaler the gradients are expected scaled by `loss_scale` as it stood when they were computed; the norm
        returned is that of the unscaled gradients, and an applying call leaves the next step's scale in `loss_scale`."""
        if self.device.type != "cuda":
            raise RuntimeError("CPU not supported")      # like the native ops: no CPU path in the product
        ext = _ext()
        tab = self._table(torch.cuda.is_current_stream_capturing())
        if tab.nrec == 0:
            return self.grad_total_norm
        lib, ng = ext._lib0, len(self.param_groups)
        accum, teacher = self.accum_steps > 1, self._teacher is not None
        # 1. squared-norm partials (accumulating: of the running sum, which it also stores)
        if accum:
            ext._run(lib.omnipq_adamw_accum_sqnorm, self.result, tab.nrec, tab.nchunks, _ptr(tab.records), _ptr(tab.chunks),
                     self.chunk_elems, _ptr(self._hyper), ng, _ptr(self.exp_avg), _ptr(self.acc), _ptr(self.accum),
                     _ptr(tab.partials))
        else:
            ext._run(lib.omnipq_adamw_grad_sqnorm, self.result, tab.nrec, tab.nchunks, _ptr(tab.records), _ptr(tab.chunks),
                     self.chunk_elems, _ptr(self._hyper), ng, _ptr(tab.partials))
        # 2. finalise: with a loss scaler the superset entry point serves every family (accum / ema_state are None where the
        # family has none); without one, the entry point of the family, as before
        if self.loss_scaler is not None:
            ext._run(lib.omnipq_adamw_scaled_finalize, self.result, tab.nchunks, _ptr(tab.partials), _ptr(self._hyper), ng,
                     self.accum_steps, _ptr(self.counters), _ptr(self.accum), _ptr(self.ema_state), _ptr(self.ema_coef),
                     _ptr(self._hyper[ng + 1]), _ptr(self.scaler_state), _ptr(self.result), _ptr(self._coef))
        elif teacher:
            ext._run(lib.omnipq_adamw_ema_finalize, self.result, tab.nchunks, _ptr(tab.partials), _ptr(self._hyper), ng,
                     self.accum_steps, _ptr(self.counters), _ptr(self.accum), _ptr(self.ema_state), _ptr(self.result),
                     _ptr(self._coef), _ptr(self.ema_coef))
        elif accum:
            ext._run(lib.omnipq_adamw_accum_finalize, self.result, tab.nchunks, _ptr(tab.partials), _ptr(self._hyper), ng,
                     self.accum_steps, _ptr(self.counters), _ptr(self.accum), _ptr(self.result), _ptr(self._coef))
        else:
            ext._run(lib.omnipq_adamw_finalize, self.result, tab.nchunks, _ptr(tab.partials), _ptr(self._hyper), ng,
                     _ptr(self.counters), _ptr(self.result), _ptr(self._coef))
        # 3. update (with a teacher: and its averaging; accum is None in the plain family)
        if teacher:
            ext._run(lib.omnipq_adamw_ema_update, self.result, tab.nrec, tab.nchunks, _ptr(tab.records), _ptr(tab.ema_ptrs),
                     _ptr(tab.chunks), self.chunk_elems, tab.n_only, tab.n_only_chunks, _ptr(tab.ema_only),
                     _ptr(tab.only_chunks), _ptr(self.exp_avg), _ptr(self.acc), _ptr(self.accum), _ptr(self._coef),
                     _ptr(self.ema_coef), _ptr(self.result))
        elif accum:
            ext._run(lib.omnipq_adamw_accum_update, self.result, tab.nrec, tab.nchunks, _ptr(tab.records), _ptr(tab.chunks),
                     self.chunk_elems, _ptr(self.exp_avg), _ptr(self.acc), _ptr(self.accum), _ptr(self._coef),
                     _ptr(self.result))
        else:
            ext._run(lib.omnipq_adamw_update, self.result, tab.nrec, tab.nchunks, _ptr(tab.records), _ptr(tab.chunks),
                     self.chunk_elems, _ptr(self._coef), _ptr(self.result))
        if accum:
            self.replayed()
        else:
            self._applied = True
        return self.grad_total_norm

    @torch.no_grad()
    def step(self, closure=None):
        """clip_grad_norm_(max_norm) + AdamW.step() in three launches.  -> grad_total_norm, a 0-dim DEVICE tensor (the norm of
        grad_scale * gradients before clipping -- with a loss scaler divided by the scale the gradients carry, i.e. of the
        unscaled gradients; rewritten by the next step).  Parameters whose .grad is None are left out.
        accum_steps = k > 1: call once per micro-batch.  Every call adds the gradients into the accumulator and returns the
        norm of grad_scale * the running SUM; every k-th call clips and applies that sum (`is_update_step`), the others leave
        parameters, moments and the step count alone.  The gradients are summed as in the reference, whose loss is not
        divided by step_freq: grad_scale = 1 / k gives the mean.  The set of parameters with gradients must not change
        inside one accumulation; their gradients' addresses may."""
        if closure is not None:
            raise NotImplementedError("FusedAdamW.step: closures are not supported")
        if self.device.type != "cuda":
            raise RuntimeError("CPU not supported")
        self.sync_hyperparameters()
        return self.launch()

    # ---- save / restore (CapturedStep's warm-up and capture runs must leave no trace) ---------------------------------------
    def _saved_tensors(self):
        return (self.exp_avg, self.exp_avg_sq, self.counters, self.result) + \
            ((self.scaler_state,) if self.loss_scaler is not None else ()) + \
            ((self.acc, self.accum) if self.accum_steps > 1 else ()) + \
            ((self.ema_state, self.ema_coef) + tuple(e for e, _ in self._teacher) if self._teacher is not None else ())

    def snapshot(self):
        """moments, counters and -- the warm-up and capture runs advance them too -- the accumulator, the device micro-batch
        counter and its host mirror; with a teacher attached its global_step, coefficients and weights as well; with a loss
        scaler its scale and growth tracker"""
        return [t.detach().clone() for t in self._saved_tensors()] + [(self._micro, self._applied)]

    def restore(self, saved):
        tensors = self._saved_tensors()
        if len(tensors) != len(saved) - 1:
            raise RuntimeError("FusedAdamW.restore: a teacher was attached or detached since the snapshot was taken")
        with torch.no_grad():
            for t, s in zip(tensors, saved):
                t.copy_(s)
        self._micro, self._applied = saved[-1]
