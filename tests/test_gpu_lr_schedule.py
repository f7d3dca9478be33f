"""The learning-rate schedule on the GPU (optim.LRSchedule, FusedAdamW(lr_schedule=...); include/omnipq_optim.h:
omnipq_lr_schedule_eval, omnipq_adamw_sched_finalize) against tests/lr_schedule_restatement.py, against a twin optimiser that is
fed the same rates from the host, captured and replayed, resumed from its state dicts -- and the finalise entry points that were
there before, which share the kernel body, against a float64 emulation of the header's formulas.

The cosine bound (tests 1 and 3).  Host and device evaluate eta_min + (b - eta_min) * (1 + cos(x)) / 2 on the SAME x = pi * k /
T_max (two IEEE operations, identical bits) and differ only in cos.  The device's math library is written to the OpenCL C
specification, whose table of relative errors (section 7.4, "Relative Error as ULPs") allows cos 4 ulp in double precision; taken
at twice that, 8 ulp, plus the 1 ulp the GNU C library documents for its own cos (glibc manual, "Known Maximum Errors in Math
Functions"), two values of cos(x) differ by at most 9 * 2^-52 (|cos| <= 1).  Every rounding below is at most 2^-53 relative to
its result, on the host and on the device alike, so a pair of them separates the two sides by at most 2^-52 of the result's size:
    s = 1 + cos(x)          s <= 2:              |ds| <= 9 * 2^-52 + 2 * 2^-52              = 11   * 2^-52
    p = (b - eta_min) * s   p <= 2 b:            |dp| <= b * 11 * 2^-52 + 2 b * 2^-52       = 13   * 2^-52 * b
    q = p / 2               exact:               |dq|                                       =  6.5 * 2^-52 * b
    lr = eta_min + q        lr <= b:             |dlr| <= 6.5 * 2^-52 * b + b * 2^-52       =  7.5 * 2^-52 * b
(b - eta_min itself has identical operands on both sides.)  So |lr_device - lr_host| <= 7.5 * 2^-52 * b <= 2^-49 * b, the bound
asserted.  Everything else in the schedule is +, -, *, / on identical operands: bit-equal.
"""
import copy
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, HERE)

import lr_schedule_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

COS_BOUND = 2.0 ** -49                      # relative to the base rate: see the head of this file
LRS = R.BASE_LRS
SIZES = (1, 1031, 2048)                     # one element, no multiple of four, one aligned tile
GROUP = (0, 1, 0)
CALLS = 24
# W = 6 and, for the step schedule, a milestone at k = 10 (e = 16): 24 steps cross both
TOY = dict(n_iter_per_epoch=2, max_epoch=20, warmup_epoch=3, warmup_multiplier=100, lr_decay_epochs=(8,), lr_decay_rate=0.1)


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def _schedule(kind, **over):
    import optim
    kw = dict(TOY, **over)
    return optim.LRSchedule(kind, kw.pop("n_iter_per_epoch"), kw.pop("max_epoch"), **kw)


def _restated(kind, **over):
    kw = dict(TOY, **over)
    return R.Schedule(kind, kw.pop("n_iter_per_epoch"), kw.pop("max_epoch"), **kw)


# ---- 1. the evaluation launch -------------------------------------------------------------------------------------------------

EVAL_CASES = [(name, dict(n_iter_per_epoch=R.N_ITER, max_epoch=R.MAX_EPOCH, warmup_epoch=warm, warmup_multiplier=R.MULTIPLIER,
                          lr_decay_epochs=R.DECAY_EPOCHS, lr_decay_rate=R.DECAY_RATE), kind)
              for name, (kind, warm) in R.CASES.items()]
EVAL_CASES += [
    ("W=1, milestone at k=0", dict(n_iter_per_epoch=1, max_epoch=12, warmup_epoch=1, lr_decay_epochs=(1, 3)), "step"),
    ("milestone at k=0, no warm-up", dict(n_iter_per_epoch=2, max_epoch=5, warmup_epoch=-1, lr_decay_epochs=(-1, 1),
                                          lr_decay_rate=0.5), "step"),
    ("duplicate milestones", dict(n_iter_per_epoch=1, max_epoch=20, warmup_epoch=-1, lr_decay_epochs=(3, 3, 6)), "step"),
    ("eight milestones", dict(n_iter_per_epoch=1, max_epoch=20, warmup_epoch=2, lr_decay_epochs=tuple(range(3, 11)),
                              lr_decay_rate=0.7), "step"),
    ("T_max=1", dict(n_iter_per_epoch=1, max_epoch=0, warmup_epoch=-1), "cosine"),
    ("e > T_max", dict(n_iter_per_epoch=3, max_epoch=9, warmup_epoch=2), "cosine"),
]


def _tiny_optimizer(dev, sched):
    import optim
    params = [torch.nn.Parameter(torch.zeros(4, device=dev)) for _ in LRS]
    return optim.FusedAdamW([{"params": [p], "lr": lr} for p, lr in zip(params, LRS)], lr_schedule=sched)


@pytest.mark.parametrize("name,kw,kind", EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_eval_launch_is_the_restatement(name, kw, kind):
    """1: omnipq_lr_schedule_eval for e = 0..99, two groups: warm-up values and every step-schedule value bit for bit, cosine
    values within COS_BOUND * base rate"""
    dev = torch.device("cuda", 0)
    s = _schedule(kind, **kw)
    restated = _restated(kind, **kw)
    opt = _tiny_optimizer(dev, s)
    assert opt.staged == 1
    got = []
    for e in range(100):
        s.set_last_epoch(e)                       # the device word, then one evaluation launch
        got.append(s.lr_now.clone())
    got = torch.stack(got).cpu().numpy()
    want = np.asarray([restated.lrs(e, LRS) for e in range(100)])
    warm = np.arange(100) <= restated.warmup_iters if restated.warmup_iters > 0 else np.zeros(100, dtype=bool)
    assert got[warm].tobytes() == want[warm].tobytes(), np.argwhere(got[warm] != want[warm])[:4]
    if kind == "step":
        assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
        assert len(np.unique(want[:, 0])) >= 2
    else:
        err = np.abs(got - want) / np.asarray(LRS)
        print(f"{name}: max |device - restatement| / base rate = {err.max():.3e}, bound {COS_BOUND:.3e}")
        assert (err <= COS_BOUND).all(), (np.argwhere(err > COS_BOUND)[:4], err.max())
    assert opt.staged == 1 and s.last_epoch == 99


# ---- 2. the toy model -----------------------------------------------------------------------------------------------------------

class Toy(torch.nn.Module):
    """three f32 tensors of 1, 1031 and 2048 elements; the second is a view one element into a buffer: 4 bytes off a 16-byte
    boundary"""

    def __init__(self, dev):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.buffer = torch.randn(SIZES[1] + 8, generator=g).to(dev)
        vals = [torch.randn(n, generator=g) for n in SIZES]
        ps = [torch.nn.Parameter(vals[0].to(dev)), torch.nn.Parameter(self.buffer[1:1 + SIZES[1]]),
              torch.nn.Parameter(vals[2].to(dev))]
        with torch.no_grad():
            ps[1].copy_(vals[1])
        assert ps[1].data_ptr() % 16 == 4 and ps[2].data_ptr() % 16 == 0
        self.ps = torch.nn.ParameterList(ps)


def _grads(i, bad=None):
    g = torch.Generator().manual_seed(500 + i)
    out = [torch.randn(n, generator=g) * (3e-2 if i % 3 else 1e-3) for n in SIZES]        # norms 1.7 and 0.055: both sides of max_norm
    if bad == i:
        out[1][5] = float("inf")
    return out


def _build(dev, kind, with_schedule, accum=1, everything=False):
    import optim
    net = Toy(dev)
    params = list(net.ps)
    sched = _schedule(kind) if with_schedule else None
    kw = {}
    if everything:
        kw["loss_scaler"] = optim.LossScaler(init_scale=2.0 ** 4, growth_interval=3)
    opt = optim.FusedAdamW([{"params": [p for p, gi in zip(params, GROUP) if gi == g], "lr": LRS[g]} for g in (0, 1)],
                           betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, max_norm=0.1, accum_steps=accum, lr_schedule=sched,
                           **kw)
    teacher = None
    if everything:
        teacher = copy.deepcopy(net)
        for p in teacher.parameters():
            p.requires_grad_(False)
        opt.attach_teacher(net, teacher, 0.9)
    keep = [torch.zeros_like(p) for p in params]
    for p, k in zip(params, keep):
        p.grad = k
    return net, params, opt, sched, teacher, keep


def _state(params, opt, teacher):
    out = [p.detach().clone() for p in params] + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.counters.clone()]
    if teacher is not None:
        out += [p.detach().clone() for p in teacher.parameters()] + [opt.ema_state.clone(), opt.scaler_state.clone()]
    return out


def _run(dev, kind, feed=None, accum=1, bad=None, everything=False, first=0, calls=CALLS, built=None):
    """-> (lr_now in front of every call, lr_now behind every call, state behind every call, the objects).  feed: None = the
    schedule on the device; else the rates to write into param_groups in front of each call (no schedule attached)."""
    net, params, opt, sched, teacher, keep = built or _build(dev, kind, feed is None, accum, everything)
    before, after, states = [], [], []
    for i in range(first, calls):
        for k, g in zip(keep, _grads(i, bad)):
            k.copy_(g)
        if feed is None:
            before.append(sched.lr_now.clone())
        else:
            for g, lr in zip(opt.param_groups, feed[i - first]):
                g["lr"] = lr
        opt.step()
        if feed is None:
            after.append(sched.lr_now.clone())
        states.append(_state(params, opt, teacher))
    torch.cuda.synchronize()
    before = [b.cpu().tolist() for b in before]
    after = [a.cpu().tolist() for a in after]
    return before, after, states, (net, params, opt, sched, teacher, keep)


def _assert_same_states(a, b, what):
    assert len(a) == len(b)
    for i, (sa, sb) in enumerate(zip(a, b)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert torch.equal(x, y), f"{what}: call {i + 1}, tensor {j}: {(x != y).sum().item()} elements differ"


@pytest.mark.parametrize("kind", ["cosine", "step"])
def test_toy_run_equals_a_twin_fed_from_the_host(kind):
    """2: 24 steps across e = W and a milestone; p, exp_avg, exp_avg_sq, t and skipped bit-equal after every step to a twin
    without a schedule whose param_groups carry the rates read back from lr_now; the rates themselves are the restatement's"""
    dev = torch.device("cuda", 0)
    before, after, states, (_, _, opt, sched, _, _) = _run(dev, kind)
    restated = _restated(kind)
    assert sched.last_epoch == CALLS and int(sched.state) == CALLS and opt.t == CALLS and opt.staged == 1
    assert [g["lr"] for g in opt.param_groups] == list(LRS)                    # param_groups keeps the base rates
    want = [restated.lrs(e, LRS) for e in range(CALLS + 1)]
    if kind == "step":
        assert _bits(before) == _bits(want[:-1]) and _bits(after) == _bits(want[1:])
        assert want[6] != want[7] and want[15][0] != want[16][0]                # the end of the warm-up and the milestone
    else:
        assert _bits(before[:7]) == _bits(want[:7])
        err = np.abs(np.asarray(before + after[-1:]) - np.asarray(want)) / np.asarray(LRS)
        assert (err <= COS_BOUND).all(), err.max()
    assert _bits(before[1:]) == _bits(after[:-1])
    _, _, twin, (_, _, topt, _, _, _) = _run(dev, kind, feed=before)
    assert topt.staged > 7 and topt.lr_schedule is None            # the twin staged its rows whenever the rate moved
    _assert_same_states(states, twin, kind)
    assert not torch.equal(states[0][1], states[-1][1])


def test_toy_run_with_accumulation_advances_once_per_window():
    """2, accum_steps = 3: e advances on the third call of each window, lr_now stays on the other two"""
    dev = torch.device("cuda", 0)
    before, after, states, (_, _, opt, sched, _, _) = _run(dev, "step", accum=3)
    restated = _restated("step")
    assert sched.last_epoch == CALLS // 3 == int(sched.state) and opt.t == CALLS // 3
    for i in range(CALLS):
        assert _bits(before[i]) == _bits(restated.lrs(i // 3, LRS)), i
        assert _bits(after[i]) == _bits(restated.lrs((i + 1) // 3, LRS)), i
    _, _, twin, _ = _run(dev, "step", feed=before, accum=3)
    _assert_same_states(states, twin, "accum_steps=3")


def test_toy_run_counts_a_skipped_step():
    """2, one non-finite gradient: the schedule advances (train.py:566 does not look at the norm), t does not"""
    dev = torch.device("cuda", 0)
    before, after, states, (_, _, opt, sched, _, _) = _run(dev, "step", bad=8)
    restated = _restated("step")
    assert sched.last_epoch == CALLS == int(sched.state) and opt.t == CALLS - 1 and opt.skipped == 1
    assert _bits(after) == _bits([restated.lrs(e, LRS) for e in range(1, CALLS + 1)])
    for x, y in zip(states[7][:5], states[8][:5]):
        assert torch.equal(x, y)                                               # the skipped step moved nothing
    _, _, twin, _ = _run(dev, "step", feed=before, bad=8)
    _assert_same_states(states, twin, "non-finite step")


def test_toy_run_with_everything_attached():
    """2, the superset with everything on: loss scaler, teacher, accumulation and schedule in one finalise launch, against the
    twin on omnipq_adamw_scaled_finalize with the rates fed from the host"""
    dev = torch.device("cuda", 0)
    before, after, states, (_, _, opt, sched, teacher, _) = _run(dev, "cosine", accum=2, bad=9, everything=True)
    assert sched.last_epoch == CALLS // 2 == int(sched.state) and opt.skipped == 1 and opt.t == CALLS // 2 - 1
    assert opt.global_step == 1 + CALLS // 2 and opt.scale_value != 2.0 ** 4
    _, _, twin, (_, _, topt, _, _, _) = _run(dev, "cosine", feed=before, accum=2, bad=9, everything=True)
    assert topt.lr_schedule is None
    _assert_same_states(states, twin, "everything")


# ---- 3. captured --------------------------------------------------------------------------------------------------------------

def test_captured_launch_follows_the_schedule():
    """3: the toy step captured once (single stream) and replayed 24 times: the lr_now sequence and every state are the eager
    run's, nothing is staged during the replays, and a field of the device struct changed between replays takes effect on the
    next one"""
    dev = torch.device("cuda", 0)
    before, after, states, _ = _run(dev, "cosine")
    net, params, opt, sched, _, keep = _build(dev, "cosine", True)
    saved = opt.snapshot(), [p.detach().clone() for p in params]
    for k, g in zip(keep, _grads(0)):
        k.copy_(g)
    opt.step()                                    # builds the tables the captured launches read
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.launch()
    opt.restore(saved[0])
    with torch.no_grad():
        for p, q in zip(params, saved[1]):
            p.copy_(q)
    assert sched.last_epoch == 0 and int(sched.state) == 0
    staged, builds = opt.staged, opt.table_builds
    seen, replayed = [], []
    for i in range(CALLS):
        for k, g in zip(keep, _grads(i)):
            k.copy_(g)
        opt.sync_hyperparameters()                # what CapturedStep.step does in front of its replay: nothing to send
        graph.replay()
        opt.replayed()
        seen.append(sched.lr_now.clone())
        replayed.append(_state(params, opt, None))
    torch.cuda.synchronize()
    assert opt.staged == staged and opt.table_builds == builds
    assert _bits([x.cpu().tolist() for x in seen]) == _bits(after)
    _assert_same_states(states, replayed, "replay")
    assert sched.last_epoch == CALLS == int(sched.state)
    # t_max in the DEVICE struct: the next replay evaluates lr_now with it
    old = sched.get_last_lr()
    sched.field("t_max").fill_(11)
    graph.replay()
    opt.replayed()
    got = sched.get_last_lr()
    want = _restated("cosine")
    want.t_max = 11
    err = np.abs(np.asarray(got) - np.asarray(want.lrs(CALLS + 1, LRS))) / np.asarray(LRS)
    assert (err <= COS_BOUND).all(), err
    unchanged = _restated("cosine").lrs(CALLS + 1, LRS)
    assert abs(got[0] - unchanged[0]) > 1e-2 * LRS[0] and got != old


# ---- 4. resume ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["cosine", "step"])
def test_resume_from_the_state_dicts(kind):
    """4: state_dict() of schedule and optimiser at step 9, fresh objects, load_state_dict, 15 more steps: the 24 uninterrupted
    steps bit for bit"""
    dev = torch.device("cuda", 0)
    _, after, states, whole = _run(dev, kind)
    _, _, _, (net, params, opt, sched, _, _) = _run(dev, kind, calls=9)
    sd, od, weights = copy.deepcopy(sched.state_dict()), copy.deepcopy(opt.state_dict()), [p.detach().clone() for p in params]
    assert sd["last_epoch"] == 9 and sd["after_scheduler"]["last_epoch"] == 3
    built = _build(dev, kind, True)
    _, params2, opt2, sched2, _, _ = built
    with torch.no_grad():
        for p, q in zip(params2, weights):
            p.copy_(q)
    opt2.load_state_dict(od)
    sched2.load_state_dict(sd)
    assert sched2.last_epoch == 9 and int(sched2.state) == 9 and opt2.t == 9
    assert _bits(sched2.get_last_lr()) == _bits(after[8])
    _, after2, states2, _ = _run(dev, kind, first=9, built=built)
    assert _bits(after2) == _bits(after[9:])
    _assert_same_states(states[9:], states2, f"resumed {kind}")
    assert sched2.state_dict() == whole[3].state_dict() and sched2.last_epoch == CALLS


# ---- 5. the finalise entry points that were there before ---------------------------------------------------------------------------

def _emulate(partials, hyper, ng, counters, accum=None, accum_steps=1, ema_state=None, scaler=None, result=None):
    """include/omnipq_optim.h's finalise in numpy: f64 where the header says f64, f32 where it says f32.  -> (result, coef or None,
    ema_coef or None); counters, accum, ema_state and scaler are updated in place."""
    f32 = np.float32
    s = float(np.sum(partials))                    # exact: the partials are small dyadic numbers
    last = hyper[ng]
    max_norm, gs = f32(last[0]), f32(last[1])
    total = f32(math.sqrt(s))
    if scaler is not None:
        scale = f32(scaler["scale"])
        inv = 1.0 / float(scale)
        with np.errstate(over="ignore"):
            total, gs = f32(math.sqrt(s) * inv), f32(last[1] * inv)
    finite = bool(np.isfinite(total))
    result = np.array(result, dtype=np.float32)
    if accum is not None:
        if 0 <= accum[0] < accum_steps - 1:
            result[0] = total
            accum[0] += 1
            accum[1] = 0
            return result, None, None
        accum[0], accum[1] = 0, 1
    ema_coef = None
    if ema_state is not None:
        a = min(1.0 - 1.0 / float(ema_state[0] + 1), last[2])
        ema_coef = np.array([f32(a), f32(1.0 - a)], dtype=np.float32)
        ema_state[0] += 1
    if scaler is not None:
        growth, backoff, interval = scaler["cfg"]
        if not finite:
            scaler["scale"], scaler["tracker"] = f32(float(scale) * backoff), 0
        elif scaler["tracker"] + 1 == int(interval):
            grown = f32(float(scale) * growth)
            if np.isfinite(grown):
                scaler["scale"] = grown
            scaler["tracker"] = 0
        else:
            scaler["tracker"] += 1
    clip = f32(1.0)
    if max_norm > 0 and finite:
        clip = min(f32(1.0), max_norm / (total + f32(1e-6)))
    result[:] = (total, clip, 0.0 if finite else 1.0, gs * clip)
    if not finite:
        counters[1] += 1
        return result, None, ema_coef
    counters[0] += 1
    t = float(counters[0])
    coef = np.zeros((ng, 8), dtype=np.float32)
    for g in range(ng):
        lr, b1, b2, eps, wd = hyper[g][:5]
        coef[g] = (1.0 - lr * wd, b1, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), eps)
    return result, coef, ema_coef


@pytest.mark.parametrize("family", ["plain", "accum", "ema", "ema_accum", "scaled", "scaled_ema_accum"])
def test_existing_finalize_entry_points_keep_their_bits(family):
    """5: omnipq_adamw_finalize, _accum_finalize, _ema_finalize and _scaled_finalize -- instantiations of the kernel body the
    schedule was added to -- over six calls each (clipped, unclipped, a non-finite norm, a growing and a backed-off scale)
    against the float64 emulation of the header's formulas, every output word bit for bit"""
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    lib = ext._lib0
    dev = torch.device("cuda", 0)
    ng, k = 2, (2 if "accum" in family else 1)
    ema, scaled = "ema" in family, "scaled" in family
    hyper = np.zeros((ng + 2, 8))
    hyper[0, :5] = (2e-3, 0.9, 0.999, 1e-8, 5e-4)
    hyper[1, :5] = (1e-4, 0.8, 0.99, 1e-6, 0.0)
    hyper[2, :3] = (0.1, 0.5, 0.75)
    hyper[3, :3] = (2.0, 0.5, 2.0)
    P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)     # noqa: E731
    d_hyper = torch.from_numpy(hyper).to(dev)
    d_counters = torch.tensor([4, 1], dtype=torch.int64, device=dev)
    d_accum = torch.zeros(2, dtype=torch.int64, device=dev) if k > 1 else None
    d_ema_state = torch.tensor([3], dtype=torch.int64, device=dev) if ema else None
    d_ema_coef = torch.full((2,), -1.0, device=dev) if ema else None
    d_scaler = torch.zeros(8, dtype=torch.uint8, device=dev) if scaled else None
    if scaled:
        d_scaler.view(torch.float32)[0] = 8.0
    d_result = torch.full((4,), -1.0, device=dev)
    d_coef = torch.full((ng * 8,), -1.0, device=dev)
    counters, accum = np.array([4, 1]), (np.zeros(2, dtype=np.int64) if k > 1 else None)
    ema_state = np.array([3]) if ema else None
    scaler = dict(scale=np.float32(8.0), tracker=0, cfg=hyper[3, :3]) if scaled else None
    result, coef, ema_coef = np.full(4, -1.0, dtype=np.float32), np.full((ng, 8), -1.0, dtype=np.float32), \
        np.full(2, -1.0, dtype=np.float32)
    n = 300                                                                    # more partials than one pass of 256 threads
    for call in range(6):
        partials = np.ldexp(np.arange(1, n + 1, dtype=np.float64) % 17 + 1.0, -20 + 2 * call)
        if call == 3:
            partials[7] = np.inf
        d_partials = torch.from_numpy(partials).to(dev)
        if family == "plain":
            ext._run(lib.omnipq_adamw_finalize, d_result, n, P(d_partials), P(d_hyper), ng, P(d_counters), P(d_result), P(d_coef))
        elif family == "accum":
            ext._run(lib.omnipq_adamw_accum_finalize, d_result, n, P(d_partials), P(d_hyper), ng, k, P(d_counters), P(d_accum),
                     P(d_result), P(d_coef))
        elif not scaled:
            ext._run(lib.omnipq_adamw_ema_finalize, d_result, n, P(d_partials), P(d_hyper), ng, k, P(d_counters), P(d_accum),
                     P(d_ema_state), P(d_result), P(d_coef), P(d_ema_coef))
        else:
            ext._run(lib.omnipq_adamw_scaled_finalize, d_result, n, P(d_partials), P(d_hyper), ng, k, P(d_counters), P(d_accum),
                     P(d_ema_state), P(d_ema_coef), P(d_hyper[ng + 1]), P(d_scaler), P(d_result), P(d_coef))
        r, c, e = _emulate(partials, hyper, ng, counters, accum, k, ema_state, scaler, result)
        result = r
        coef = c if c is not None else coef
        ema_coef = e if e is not None else ema_coef
        where = f"{family}, call {call + 1}"
        assert d_result.cpu().numpy().tobytes() == result.tobytes(), (where, d_result.tolist(), result.tolist())
        assert d_coef.cpu().numpy().tobytes() == coef.tobytes(), (where, d_coef.tolist(), coef.tolist())
        assert d_counters.tolist() == counters.tolist(), where
        if k > 1:
            assert d_accum.tolist() == accum.tolist(), where
        if ema:
            assert d_ema_state.tolist() == ema_state.tolist() and d_ema_coef.cpu().numpy().tobytes() == ema_coef.tobytes(), where
        if scaled:
            assert d_scaler.view(torch.float32)[0].item() == float(scaler["scale"]), where
            assert d_scaler.view(torch.int32)[1].item() == scaler["tracker"], where
    assert counters.tolist() == [9, 2] if k == 1 else counters.tolist() == [6, 2]      # the non-finite call was an applying one
