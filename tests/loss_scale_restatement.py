"""The dynamic loss scale of include/omnipq_optim.h (omnipq_adamw_scaled_finalize) restated in float64 on the CPU: the `Truth`
recurrence of test_gpu_fused_adamw.py extended by the scale S and its growth tracker, plus the fixed gradient schedule that
walks every branch of the recurrence.  tests/test_loss_scale_host.py holds this restatement to torch itself without a GPU
(torch._amp_update_scale_, and torch.amp.GradScaler("cpu") + clip_grad_norm_ + torch.optim.AdamW); tests/test_gpu_loss_scale.py
then holds the kernels to it.

The schedule, with growth_interval = 3 (the scale after each step, from init S0):
    finite finite finite   -> S0, S0, 2 S0      the third good step grows
    inf                    -> S0                backs off, tracker = 0
    finite                 -> S0                tracker = 1
    nan                    -> S0 / 2            backs off, the tracker restarts
    finite finite finite   -> S0 / 2, S0 / 2, S0   grows again
and a second run of three finite steps from S0 = 2^127, where the candidate 2^128 is not finite in f32: growth is refused and
the tracker is reset all the same.
"""
import math

import numpy as np
import torch

from test_gpu_fused_adamw import GROUP, LRS, MAX_NORM, SCALES, Truth, make_grads

INTERVAL = 3
GROWTH, BACKOFF = 2.0, 0.5
INIT = 2.0 ** 16
SCHEDULE = ("finite", "finite", "finite", "inf", "finite", "nan", "finite", "finite", "finite")
TOP = 2.0 ** 127                     # the largest power of two whose double is not finite in f32
TOP_SCHEDULE = ("finite", "finite", "finite")
BAD_AT = (5, (17, 33))               # where the non-finite value goes: tensor 5 (288 x 2048), as in the existing skip test


def unscaled_grads(schedule=SCHEDULE):
    """the UNSCALED f32 gradients of every step (a non-finite step has them too: its poison is added after scaling).  The long
    schedule cycles through the magnitudes of the existing arithmetic test, clipped and unclipped steps alike.  The run at
    2^127 stays below max_norm (norms ~0.018 against 0.1): the update's one f32 coefficient grad_scale * clip_coef / S is
    then the power of two 2^-127 itself, which a subnormal f32 holds exactly; times a clip coefficient below 1 it would keep
    19 of its 24 bits (include/omnipq_optim.h says so), and the bound of these tests is one for full f32 precision."""
    if schedule is TOP_SCHEDULE:
        return [make_grads(i, 2e-5) for i in range(len(schedule))]
    return [make_grads(i, SCALES[i % len(SCALES)]) for i in range(len(schedule))]


def scaled(grads, scale, kind="finite"):
    """what backward() of (loss * scale) leaves in .grad: g * scale in f32, and the step's inf / nan in one element"""
    out = [None if g is None else g * scale for g in grads]
    if kind != "finite":
        t, at = BAD_AT
        out[t][at] = float(kind)
    return out


def update_scale(scale, tracker, finite, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL):
    """torch._amp_update_scale_ restated: `scale` is a Python float holding an f32 exactly; products in f64, one rounding"""
    with np.errstate(over="ignore"):
        if not finite:
            return float(np.float32(scale * backoff)), 0
        tracker += 1
        if tracker == interval:
            grown = np.float32(scale * growth)
            return (float(grown) if np.isfinite(grown) else scale), 0
        return scale, tracker


class ScaledTruth(Truth):
    """Truth + { scale, growth_tracker, skipped }.  step() takes the gradients as the kernels see them, scaled by self.scale."""

    def __init__(self, vals, init_scale=INIT, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL, lrs=LRS, max_norm=MAX_NORM,
                 grad_scale=1.0):
        super().__init__(vals, lrs=lrs, max_norm=max_norm, grad_scale=grad_scale)
        self.user_gs = grad_scale
        self.scale, self.tracker, self.skipped = float(np.float32(init_scale)), 0, 0
        self.growth, self.backoff, self.interval = growth, backoff, interval

    def step(self, grads, group=GROUP):
        """-> (norm of the unscaled gradients as an f32-rounded float, was the step applied)"""
        inv = 1.0 / self.scale
        sq = sum(float((self.user_gs * g.double()).square().sum()) for g in grads if g is not None)
        with np.errstate(over="ignore", invalid="ignore"):
            norm32 = float(np.float32(math.sqrt(sq) * inv)) if not math.isnan(sq) else float("nan")
        finite = math.isfinite(norm32)
        if finite:
            self.gs = self.user_gs * inv             # the effective factor: grad_scale / S
            super().step(grads, group)
        else:
            self.skipped += 1
        self.scale, self.tracker = update_scale(self.scale, self.tracker, finite, self.growth, self.backoff, self.interval)
        return norm32, finite
