"""The learning-rate schedule of the reference's utils/lr_scheduler.py: get_scheduler, restated in float64 (numpy and math only):
the contract of optim.LRSchedule and of the device recurrence (include/omnipq_optim.h: struct omnipq_lr_schedule).

With e = the number of scheduler.step() calls so far, W = warmup_epoch * n_iter_per_epoch and b a group's base rate:

    warmup_epoch > 0 and e <= W:   b / multiplier * ((multiplier - 1.) * e / W + 1.)       GradualWarmupScheduler.get_lr
    otherwise, k = e - W (k = e without warm-up):
      cosine:  eta_min + (b - eta_min) * (1 + cos(pi * k / T_max)) / 2                     CosineAnnealingLR's closed form
      step:    b * gamma ** bisect_right(sorted(milestones), k)                            MultiStepLR's closed form
    T_max = (max_epoch - warmup_epoch) * n_iter, eta_min = 1e-6, milestones (m - warmup_epoch) * n_iter: as get_scheduler
    forms them.

The reference passes an explicit epoch to after_scheduler.step behind a warm-up, so torch takes these closed forms and the
restatement equals it bit for bit; without a warm-up torch chains its recursive forms and drifts from them by rounding
(tests/golden/lr_schedule.npz records by how much).
"""
import math
from bisect import bisect_right

MAX_MILESTONES = 8          # what the library reports (omnipq_lr_schedule_max_milestones); the host tests hold the two equal

# the configuration of tests/golden/make_golden_lr_schedule.py
BASE_LRS = (2e-3, 1e-4)
N_ITER, MAX_EPOCH, DECAY_EPOCHS, DECAY_RATE, MULTIPLIER, STEPS = 7, 12, (6, 9), 0.1, 100, 89
CASES = {"cosine_warm": ("cosine", 2), "step_warm": ("step", 2), "cosine_cold": ("cosine", -1), "step_cold": ("step", -1)}
DICT_STEPS = (0, 14, 15, 20)


class Schedule:
    def __init__(self, kind, n_iter_per_epoch, max_epoch, warmup_epoch=-1, warmup_multiplier=100, lr_decay_epochs=(),
                 lr_decay_rate=0.1, eta_min=1e-6):
        if "cosine" in kind:
            self.kind = "cosine"
        elif "step" in kind:
            self.kind = "step"
        else:
            raise NotImplementedError(f"scheduler {kind} not supported")
        if isinstance(lr_decay_epochs, int):
            lr_decay_epochs = [lr_decay_epochs]
        self.warmup_iters = warmup_epoch * n_iter_per_epoch if warmup_epoch > 0 else 0
        self.multiplier = warmup_multiplier
        self.t_max = (max_epoch - warmup_epoch) * n_iter_per_epoch
        self.eta_min = eta_min
        self.gamma = lr_decay_rate
        self.milestones = sorted((m - warmup_epoch) * n_iter_per_epoch for m in lr_decay_epochs) if self.kind == "step" else []
        if len(self.milestones) > MAX_MILESTONES:
            raise ValueError(f"{len(self.milestones)} milestones, at most {MAX_MILESTONES}")

    def lr(self, e, b):
        w = self.warmup_iters
        k = e
        if w > 0:
            if e <= w:
                return b / self.multiplier * ((self.multiplier - 1.) * e / w + 1.)
            k = e - w
        if self.kind == "cosine":
            return self.eta_min + (b - self.eta_min) * (1 + math.cos(math.pi * k / self.t_max)) / 2
        return b * self.gamma ** bisect_right(self.milestones, k)

    def lrs(self, e, base_lrs=BASE_LRS):
        return [self.lr(e, b) for b in base_lrs]


def case(name):
    kind, warm = CASES[name]
    return Schedule(kind, N_ITER, MAX_EPOCH, warm, MULTIPLIER, DECAY_EPOCHS, DECAY_RATE)
