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

The learning-rate schedule (the reference's utils/lr_scheduler.py: get_scheduler, stepped at train.py:566):
`FusedAdamW(..., lr_schedule=LRSchedule(kind, n_iter_per_epoch, max_epoch, warmup_epoch, ...))`.  The groups' `lr` at
construction are the base rates; the finalise launch (omnipq_adamw_sched_finalize, the superset of all the others) forms its
coefficients from `lr_now` in device memory and every applying call counts one scheduler step and re-evaluates it -- warm-up,
then cosine or multi-step, in float64 and the reference's operation order.  Nothing is staged per step (`staged` counts what
sync_hyperparameters() sent), a captured launch follows the schedule by itself, and `LRSchedule.state_dict()` /
`load_state_dict()` speak the reference's scheduler dicts.  Without `lr_schedule=` a host scheduler keeps working on
`param_groups` as before.
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


class LRSchedule:
    """The schedule the reference's utils/lr_scheduler.py: get_scheduler builds (GradualWarmupScheduler in front of
    CosineAnnealingLR or MultiStepLR, stepped once per applying step: train.py:566), as a recurrence of the optimiser's finalise
    launch: `FusedAdamW(..., lr_schedule=s)`.  The configuration is one struct omnipq_lr_schedule in DEVICE memory
    (include/omnipq_optim.h states the formulas), next to the groups' base rates, the scheduler-step count `e` and `lr_now`, the
    rates of the next step; every applying launch -- a replayed one too -- forms its coefficients from lr_now, counts e += 1
    and re-evaluates lr_now.  Nothing is staged per step, and `scheduler.step()` has no place left in the loop: step() raises.

    The arguments carry get_scheduler's names (from_args() reads them off the reference's `args`); any kind it does not build
    raises its NotImplementedError.  `last_epoch` mirrors `e` on the host without a device read, like `optimizer.micro`.
    state_dict() / load_state_dict() speak the reference's dicts: GradualWarmupScheduler's with its nested after_scheduler, or
    torch's bare CosineAnnealingLR / MultiStepLR dict without a warm-up."""

    KINDS = ("cosine", "step")

    def __init__(self, kind, n_iter_per_epoch, max_epoch, warmup_epoch=-1, warmup_multiplier=100, lr_decay_epochs=(),
                 lr_decay_rate=0.1, eta_min=1e-6):
        if "cosine" in kind:
            self.kind = "cosine"
        elif "step" in kind:
            self.kind = "step"
        else:
            raise NotImplementedError(f"scheduler {kind} not supported")
        if isinstance(lr_decay_epochs, (int, np.integer)):
            lr_decay_epochs = [lr_decay_epochs]
        for name, v in (("n_iter_per_epoch", n_iter_per_epoch), ("max_epoch", max_epoch), ("warmup_epoch", warmup_epoch)):
            if not _is_int(v):
                raise ValueError(f"LRSchedule: {name} must be an integer, not {v!r}")
        self.warmup_iters = int(warmup_epoch * n_iter_per_epoch) if warmup_epoch > 0 else 0
        self.multiplier = warmup_multiplier
        self.t_max = int((max_epoch - warmup_epoch) * n_iter_per_epoch)
        self.eta_min = float(eta_min)
        self.gamma = lr_decay_rate
        self.milestones = sorted(int((m - warmup_epoch) * n_iter_per_epoch) for m in lr_decay_epochs) \
            if self.kind == "step" else []
        self.base_lrs = None
        self.last_epoch = 0
        self._opt = None
        self.sched = self.base_lr = self.state = self.lr_now = None        # device memory, once attached to a GPU optimiser
        self.validate()

    @classmethod
    def from_args(cls, args, n_iter_per_epoch):
        """The names get_scheduler reads off `args`: lr_scheduler, max_epoch, warmup_epoch, and -- where it reads them --
        warmup_multiplier (with a warm-up) and lr_decay_epochs / lr_decay_rate (step)."""
        kw = {}
        if "cosine" not in args.lr_scheduler and "step" in args.lr_scheduler:
            kw.update(lr_decay_epochs=args.lr_decay_epochs, lr_decay_rate=args.lr_decay_rate)
        if args.warmup_epoch > 0:
            kw.update(warmup_multiplier=args.warmup_multiplier)
        return cls(args.lr_scheduler, n_iter_per_epoch, args.max_epoch, args.warmup_epoch, **kw)

    @staticmethod
    def max_milestones():
        return int(_ext()._lib0.omnipq_lr_schedule_max_milestones())

    def validate(self):
        """The host copy of the device struct: what the library cannot check once it is in device memory."""
        if self.kind not in self.KINDS:
            raise ValueError(f"LRSchedule: kind must be one of {self.KINDS}, not {self.kind!r}")
        if not _is_int(self.t_max) or self.t_max < 1:
            raise ValueError(f"LRSchedule: T_max = (max_epoch - warmup_epoch) * n_iter_per_epoch must be >= 1, not {self.t_max!r}")
        if not _is_int(self.warmup_iters) or self.warmup_iters < 0:
            raise ValueError(f"LRSchedule: warmup_iters must be an integer >= 0, not {self.warmup_iters!r}")
        if self.warmup_iters > 0 and (not _is_real(self.multiplier) or not self.multiplier > 1.):
            raise ValueError("multiplier should be greater than 1.")        # GradualWarmupScheduler's own words
        if not _is_real(self.eta_min) or not math.isfinite(self.eta_min):
            raise ValueError(f"LRSchedule: eta_min must be a finite number, not {self.eta_min!r}")
        if not _is_real(self.gamma) or not math.isfinite(self.gamma):
            raise ValueError(f"LRSchedule: lr_decay_rate must be a finite number, not {self.gamma!r}")
        if list(self.milestones) != sorted(self.milestones) or not all(_is_int(m) for m in self.milestones):
            raise ValueError(f"LRSchedule: milestones must be sorted integers, not {self.milestones!r}")
        if len(self.milestones) > self.max_milestones():
            raise ValueError(f"LRSchedule: {len(self.milestones)} milestones, the library's struct omnipq_lr_schedule holds "
                             f"at most {self.max_milestones()}")

    # ---- the formulas on the host (tests/lr_schedule_restatement.py is the contract) -----------------------------------------
    def lr_at(self, e, b):
        """the rate of base rate b after e scheduler steps, in float64 and the reference's operation order"""
        w, k = self.warmup_iters, e
        if w > 0:
            if e <= w:
                return b / self.multiplier * ((self.multiplier - 1.) * e / w + 1.)
            k = e - w
        if self.kind == "cosine":
            return self.eta_min + (b - self.eta_min) * (1 + math.cos(math.pi * k / self.t_max)) / 2
        return b * self.gamma ** sum(1 for m in self.milestones if m <= k)

    # ---- the device side ---------------------------------------------------------------------------------------------------
    def _struct(self):
        rec = _ext().lr_schedule_struct()
        s = rec()
        nm = len(s.milestones)
        if len(s.gamma_pow) != nm + 1 or nm != self.max_milestones():
            raise RuntimeError("LRSchedule: the loaded library's struct omnipq_lr_schedule does not hold one power of gamma more "
                               "than milestones")
        s.kind, s.n_milestones = self.KINDS.index(self.kind), len(self.milestones)
        s.warmup_iters, s.t_max = self.warmup_iters, self.t_max
        s.multiplier, s.eta_min = float(self.multiplier), float(self.eta_min)
        for j, m in enumerate(self.milestones):
            s.milestones[j] = m
        for j in range(nm + 1):
            s.gamma_pow[j] = float(self.gamma ** j)          # Python's own pow: the step schedule keeps the host's bits
        return s

    def _attach(self, opt):
        if self._opt is not None and self._opt is not opt:
            raise ValueError("LRSchedule: already attached to another optimiser (its step count lives in that optimiser's launches)")
        self._opt = opt
        self.base_lrs = [float(g["lr"]) for g in opt.param_groups]
        if opt.device.type != "cuda":
            return
        rec = _ext().lr_schedule_struct()
        self.sched = torch.zeros(ctypes.sizeof(rec), dtype=torch.uint8, device=opt.device)
        self.base_lr = torch.tensor(self.base_lrs, dtype=torch.float64, device=opt.device)
        self.state = torch.full((1,), int(self.last_epoch), dtype=torch.int64, device=opt.device)
        self.lr_now = torch.zeros(len(self.base_lrs), dtype=torch.float64, device=opt.device)
        self.upload()

    def upload(self):
        """Validate the host copy, write it into the device struct and re-evaluate lr_now there (one small launch), all on the
        current stream: a captured launch sees the change on its next replay."""
        self.validate()
        if self.sched is None:
            return
        raw = np.frombuffer(bytes(self._struct()), dtype=np.uint8).copy()
        with torch.no_grad():
            self.sched.copy_(torch.from_numpy(raw))
        self._eval()

    def _eval(self):
        ext = _ext()
        ext._run(ext._lib0.omnipq_lr_schedule_eval, self.lr_now, len(self.base_lrs), _ptr(self.sched), _ptr(self.base_lr),
                 _ptr(self.state), _ptr(self.lr_now))

    def field(self, name):
        """A 0-dim (or 1-dim, for the two arrays) view of one field of the DEVICE struct: what is written through it is what the
        next launch reads.  Nothing checks such a write; upload() is the checked way."""
        if self.sched is None:
            raise RuntimeError("LRSchedule.field: not attached to an optimiser on a GPU")
        rec = _ext().lr_schedule_struct()
        f = getattr(rec, name)
        dtype = {"kind": torch.int32, "n_milestones": torch.int32, "multiplier": torch.float64, "eta_min": torch.float64,
                 "gamma_pow": torch.float64}.get(name, torch.int64)
        v = self.sched[f.offset:f.offset + f.size].view(dtype)
        return v.reshape(()) if v.numel() == 1 else v

    def _need_attached(self, what):
        if self.base_lrs is None:
            raise RuntimeError(f"LRSchedule.{what}: not attached yet -- the base rates are the groups' `lr` of "
                               "FusedAdamW(..., lr_schedule=this)")

    def get_last_lr(self):
        """the rates the NEXT applying step uses, per group -- what param_groups shows after the reference's scheduler.step().
        Reads lr_now back from the device (on an optimiser without a GPU: the same formulas on the host)."""
        self._need_attached("get_last_lr")
        if self.lr_now is not None:
            return [float(x) for x in self.lr_now.cpu().tolist()]
        return [self.lr_at(self.last_epoch, b) for b in self.base_lrs]

    def set_last_epoch(self, e):
        """Continue from scheduler step e (a resumed run): the device word, lr_now and the host mirror."""
        if not _is_int(e) or e < 0:
            raise ValueError(f"LRSchedule.set_last_epoch: an integer >= 0, not {e!r}")
        self.last_epoch = int(e)
        if self.state is not None:
            with torch.no_grad():
                self.state.fill_(int(e))
            self._eval()

    def step(self, epoch=None):
        raise RuntimeError("LRSchedule.step: this schedule is stepped on the device, by every applying launch of the optimiser "
                           "it is attached to (FusedAdamW(lr_schedule=...)) -- a host-side step would count twice")

    # ---- the reference's dicts ---------------------------------------------------------------------------------------------
    def _inner_config(self):
        if self.kind == "cosine":
            return {"T_max": self.t_max, "eta_min": self.eta_min}
        from collections import Counter
        return {"milestones": Counter(self.milestones), "gamma": self.gamma}

    def state_dict(self):
        """The keys and values the reference's scheduler holds after `last_epoch` steps of the same configuration:
        GradualWarmupScheduler.state_dict() with its nested after_scheduler (a warm-up), torch's CosineAnnealingLR /
        MultiStepLR state_dict() (none).  The outer `_last_lr` stays at the last warm-up value, as the reference leaves it."""
        self._need_attached("state_dict")
        e, w = self.last_epoch, self.warmup_iters
        flags = {"_get_lr_called_within_step": False, "_is_initial": False}
        now = self.get_last_lr()
        if w == 0:
            return dict(self._inner_config(), base_lrs=list(self.base_lrs), last_epoch=e, _step_count=e + 1, _last_lr=now, **flags)
        k = max(e - w, 0)
        inner = dict(self._inner_config(), base_lrs=list(self.base_lrs), last_epoch=k, _step_count=k + 1,
                     _last_lr=now if k > 0 else list(self.base_lrs), **flags)
        warm = min(e, w)
        return dict(multiplier=self.multiplier, warmup_epoch=w, finished=False, base_lrs=list(self.base_lrs), last_epoch=e,
                    _step_count=warm + 1, _last_lr=[self.lr_at(warm, b) for b in self.base_lrs], after_scheduler=inner, **flags)

    def load_state_dict(self, state_dict):
        """Take `last_epoch` from one of the reference's dicts after checking every configuration field it carries (T_max,
        eta_min, milestones, gamma, multiplier, warmup_epoch, base_lrs) against this schedule's own; a mismatch raises and
        changes nothing.  The dict is not modified."""
        self._need_attached("load_state_dict")
        from collections import Counter

        def check(d, name, mine):
            if name not in d:
                return
            theirs = d[name]
            if name == "milestones":
                theirs = sorted(Counter(theirs).elements()) if isinstance(theirs, dict) else sorted(theirs)
                mine = list(self.milestones)
            elif name == "base_lrs":
                theirs = [float(x) for x in theirs]
            if theirs != mine:
                raise ValueError(f"LRSchedule.load_state_dict: the state was written with {name} = {d[name]!r}, this schedule "
                                 f"has {mine!r}")

        inner = state_dict.get("after_scheduler")
        bare = state_dict if inner is None else inner
        if (inner is not None) != (self.warmup_iters > 0):
            raise ValueError("LRSchedule.load_state_dict: the state was written " +
                             ("with" if inner is not None else "without") + " a warm-up, this schedule has " +
                             (f"one of {self.warmup_iters} steps" if self.warmup_iters > 0 else "none"))
        if ("T_max" in bare) != (self.kind == "cosine") or ("milestones" in bare) != (self.kind == "step"):
            raise ValueError(f"LRSchedule.load_state_dict: the state is not that of a {self.kind} schedule")
        for d in (state_dict, bare):
            check(d, "base_lrs", list(self.base_lrs))
        check(state_dict, "multiplier", self.multiplier)
        check(state_dict, "warmup_epoch", self.warmup_iters)
        check(bare, "T_max", self.t_max)
        check(bare, "eta_min", self.eta_min)
        check(bare, "milestones", None)
        check(bare, "gamma", self.gamma)
        e = state_dict["last_epoch"]
        if not _is_int(e) or e < 0:
            raise ValueError(f"LRSchedule.load_state_dict: last_epoch must be an integer >= 0, not {e!r}")
        if inner is not None and "last_epoch" in inner and inner["last_epoch"] != max(e - self.warmup_iters, 0):
            raise ValueError(f"LRSchedule.load_state_dict: after_scheduler.last_epoch = {inner['last_epoch']!r} does not follow "
                             f"from last_epoch = {e} and warmup_epoch = {self.warmup_iters}")
        self.set_last_epoch(e)


class _Table:
    """The device tables of one (parameter, gradient) address set."""
    __slots__ = ("key", "shape_key", "records", "chunks", "partials", "nrec", "nchunks",
                 "ema_ptrs", "ema_only", "only_chunks", "n_only", "n_only_chunks")     # the teacher's side (attach_teacher)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_norm=0.0, grad_scale=1.0, chunk_elems=CHUNK, accum_steps=1, loss_scaler=None, lr_schedule=None):
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
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError("FusedAdamW: lr_schedule is an optim.LRSchedule or None (a torch scheduler steps from the host and "
                             "writes param_groups; it keeps working without this argument)")
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
        self.staged = 0                          # how often sync_hyperparameters() has sent rows to the device
        # the learning-rate schedule on the device: the base rates are the groups' `lr` as they stand now; from here on
        # param_groups[g]["lr"] IS the base rate and no launch reads it (the finalise launch reads lr_schedule.lr_now)
        self.lr_schedule = lr_schedule
        if lr_schedule is not None:
            lr_schedule._attach(self)
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
        if self._applied and self.lr_schedule is not None:
            self.lr_schedule.last_epoch += 1     # the applying launch counted one scheduler step

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
        if self.lr_schedule is not None:
            # a state written under a host scheduler carries the rate of its step in `lr` and the base rate in `initial_lr`;
            # here `lr` IS the base rate the device was given at construction, so a different base is refused, not staged
            for i, (g, b) in enumerate(zip(state_dict["param_groups"], self.lr_schedule.base_lrs)):
                if "initial_lr" in g and float(g["initial_lr"]) != b:
                    raise ValueError(f"FusedAdamW.load_state_dict: group {i} was written with the base rate "
                                     f"{g['initial_lr']!r}, the attached schedule has {b!r}")
        super().load_state_dict(state_dict)
        if self.lr_schedule is not None:
            for g, b in zip(self.param_groups, self.lr_schedule.base_lrs):
                g["lr"] = b                  # the schedule owns the rate: LRSchedule.load_state_dict() restores its step
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
        self.staged += 1
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
        if self.lr_schedule is not None:
            # the superset of the superset: every part optional, the rates read from lr_schedule.lr_now and advanced there
            sch, scaled = self.lr_schedule, self.loss_scaler is not None
            ext._run(lib.omnipq_adamw_sched_finalize, self.result, tab.nchunks, _ptr(tab.partials), _ptr(self._hyper), ng,
                     self.accum_steps, _ptr(self.counters), _ptr(self.accum), _ptr(self.ema_state), _ptr(self.ema_coef),
                     _ptr(self._hyper[ng + 1] if scaled else None), _ptr(self.scaler_state), _ptr(sch.sched),
                     _ptr(sch.base_lr), _ptr(sch.state), _ptr(sch.lr_now), _ptr(self.result), _ptr(self._coef))
        elif self.loss_scaler is not None:
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
        if accum or self.lr_schedule is not None:
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
            ((self.lr_schedule.state, self.lr_schedule.lr_now) if self.lr_schedule is not None else ()) + \
            ((self.ema_state, self.ema_coef) + tuple(e for e, _ in self._teacher) if self._teacher is not None else ())

    def snapshot(self):
        """moments, counters and -- the warm-up and capture runs advance them too -- the accumulator, the device micro-batch
        counter and its host mirror; with a teacher attached its global_step, coefficients and weights as well; with a loss
        scaler its scale and growth tracker; with a learning-rate schedule its step count, lr_now and the host mirror"""
        return [t.detach().clone() for t in self._saved_tensors()] + \
            [(self._micro, self._applied, self.lr_schedule.last_epoch if self.lr_schedule is not None else None)]

    def restore(self, saved):
        tensors = self._saved_tensors()
        if len(tensors) != len(saved) - 1:
            raise RuntimeError("FusedAdamW.restore: a teacher was attached or detached since the snapshot was taken")
        with torch.no_grad():
            for t, s in zip(tensors, saved):
                t.copy_(s)
        self._micro, self._applied, e = saved[-1]
        if self.lr_schedule is not None:
            self.lr_schedule.last_epoch = e
