"""Windowed step statistics on the GPU (step_stats.StepStats; include/omnipq_optim.h: omnipq_stats_accumulate) against the
reference's own arithmetic, `stat_dict[key] += x.item()` in Python floats: every criterion is BIT equality, because a slot's sum
is the sequential float64 sum of its values in call order and nothing else -- there is nothing to tolerate.
"""
import math
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

CALLS = 5


def _same(a, b):
    """two Python floats with the same bits; a NaN equals any NaN (it propagates, its payload is nobody's contract)"""
    return (math.isnan(a) and math.isnan(b)) or struct.pack("<d", a) == struct.pack("<d", b)


def _values(n, call):
    """n doubles spread over 30 binades, both signs, new with every call; entry 1 is NaN on call 2 and entry 2 is +Inf on call
    3 (where n has them)"""
    g = np.random.default_rng(1000 * n + call)
    v = (1.0 + g.random(n)) * np.exp2(g.integers(-15, 15, n)) * np.where(g.random(n) < 0.5, -1.0, 1.0)
    if n >= 3:
        if call == 2:
            v[1] = np.nan
        if call == 3:
            v[2] = np.inf
    return v


class Sources:
    """n device scalars as 0-dim views of two backing tensors: every third entry is a float64, the others float32"""

    def __init__(self, n, dev):
        self.n = n
        self.f32 = torch.zeros(n, dtype=torch.float32, device=dev)
        self.f64 = torch.zeros(n, dtype=torch.float64, device=dev)
        self.is64 = [i % 3 == 2 for i in range(n)]
        self.names = [f"loss_{i}" if i % 2 else f"acc_ratio_{i}" for i in range(n)]
        self.mapping = {k: (self.f64[i] if self.is64[i] else self.f32[i]) for i, k in enumerate(self.names)}
        self.mapping["center"] = torch.zeros(3, device=dev)                   # not selected
        self.last = (self.names[-1],)                                          # one entry in `last` mode

    def write(self, values):
        """-> the values as the device holds them (float32 entries rounded), as Python floats"""
        with np.errstate(over="ignore", invalid="ignore"):
            v32 = values.astype(np.float32)
        self.f32.copy_(torch.from_numpy(v32))
        self.f64.copy_(torch.from_numpy(values))
        return [float(values[i]) if self.is64[i] else float(v32[i]) for i in range(self.n)]

    def fresh(self):
        """the same scalars in newly allocated tensors"""
        out = Sources.__new__(Sources)
        out.__dict__.update(self.__dict__)
        out.f32, out.f64 = self.f32.clone(), self.f64.clone()
        out.mapping = {k: (out.f64[i] if self.is64[i] else out.f32[i]) for i, k in enumerate(self.names)}
        return out


def _python_sums(rows, last_index):
    """the reference's arithmetic: one Python-float `+=` per step, in order; the `last` entry keeps its latest value"""
    sums = [0.0] * len(rows[0])
    for row in rows:
        for i, x in enumerate(row):
            sums[i] = x if i == last_index else sums[i] + x
    return sums


def _check(window, src, rows, steps, calls):
    want = _python_sums(rows, src.n - 1)
    assert (window.steps, window.calls) == (steps, calls)
    assert list(window) == src.names
    for i, k in enumerate(src.names):
        assert _same(window[k], want[i]), (k, window[k], want[i])
        assert _same(window.last[k], rows[-1][i]), (k, window.last[k], rows[-1][i])


@pytest.mark.parametrize("n", [1, 3, 257, 1024])
def test_sums_are_the_sequential_python_float_sums(n):
    """five eager calls with changing values (mixed f32 / f64 sources, 30 binades, one NaN, one Inf, one `last` entry): sums,
    last values and the window bit for bit; one table upload (the addresses are fixed), one copy per read(); after
    read(reset=True) the window starts from zero; a re-targeted table (new tensors every call) gives the same sums"""
    import step_stats
    dev = torch.device("cuda", 0)
    src = Sources(n, dev)
    stats, moving = step_stats.StepStats(), step_stats.StepStats()
    rows = []
    for call in range(CALLS):
        rows.append(src.write(_values(n, call)))
        stats.accumulate(src.mapping, last=src.last)
        moving.accumulate(src.fresh().mapping, last=src.last)
    assert stats.table_uploads == 1 and moving.table_uploads == CALLS and stats.copies == 0
    kept = stats.read(reset=False)
    _check(kept, src, rows, CALLS, CALLS)
    if n >= 3:
        assert math.isnan(kept[src.names[1]]) and (n == 3 or kept[src.names[2]] == math.inf)
    window = stats.read()
    _check(window, src, rows, CALLS, CALLS)
    assert stats.copies == 2
    _check(moving.read(), src, rows, CALLS, CALLS)
    means = window.means()
    assert means[src.names[-1]] == window[src.names[-1]] and (n == 1 or _same(means[src.names[0]], window[src.names[0]] / CALLS))
    # the window starts from zero: two more calls
    rows = []
    for call in (7, 8):
        rows.append(src.write(_values(n, call)))
        stats.accumulate(src.mapping, last=src.last)
    _check(stats.read(), src, rows, 2, 2)
    assert stats.copies == 3 and stats.table_uploads == 1


def test_only_the_applying_micro_batch_accumulates():
    """an accum word driven as accum_steps = 3: two of three calls only count"""
    import step_stats
    dev = torch.device("cuda", 0)
    src = Sources(3, dev)
    src.last = ()
    accum = torch.zeros(2, dtype=torch.int64, device=dev)
    norm = torch.zeros((), dtype=torch.float32, device=dev)
    optimizer = types.SimpleNamespace(accum=accum, grad_total_norm=norm)
    stats = step_stats.StepStats()
    rows = []
    for call in range(9):
        vals = src.write(_values(3, 20 + call) if call != 4 else np.array([1.0, 2.0, 3.0]))
        norm.fill_(0.5 + call)
        accum[0], accum[1] = (call + 1) % 3, int(call % 3 == 2)                # as the finalise launch leaves the word
        stats.accumulate(src.mapping, optimizer)
        if call % 3 == 2:
            rows.append(vals + [0.5 + call])
    window = stats.read()
    assert (window.steps, window.calls) == (3, 9) and list(window) == src.names + ["grad_norm"]
    want = _python_sums(rows, 3)
    for i, k in enumerate(list(window)):
        assert _same(window[k], want[i]), (k, window[k], want[i])
    assert window["grad_norm"] == 8.5 == window.last["grad_norm"] and window.means(10)["grad_norm"] == 8.5


def test_captured_launch_replayed_with_rewritten_sources():
    """captured once, replayed seven times with the sources rewritten in between: the same sums"""
    import step_stats
    dev = torch.device("cuda", 0)
    src = Sources(257, dev)
    stats = step_stats.StepStats()
    src.write(_values(257, 0))
    stats.accumulate(src.mapping, last=src.last)           # allocates the table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats.accumulate(src.mapping, last=src.last)
    stats.retarget()
    stats.reset()
    rows = []
    for call in range(7):
        rows.append(src.write(_values(257, 40 + call)))
        graph.replay()
    _check(stats.read(), src, rows, 7, 7)
    assert stats.table_uploads == 1 and stats.copies == 1


def _model_and_optimizer(dev):
    sys.path.insert(0, REPO)
    import bench
    import optim
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    net = load_procedural(bench.build_model(0)).to(dev).train()
    zero_dropout(net)
    groups = [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
              {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": 1e-4}]
    sched = optim.LRSchedule("cosine", 2, 6, 1)
    return net, optim.FusedAdamW(groups, lr=2e-3, weight_decay=5e-4, max_norm=0.1, lr_schedule=sched), sched


class _Criterion:
    """bench.py's stand-in loss, and a few reported scalars formed by deterministic reductions of the forward's outputs"""

    def __init__(self):
        self.stats = {}

    def __call__(self, ep, labels):
        import bench
        self.stats = {"center_abs_loss": ep["last_center"].detach().float().abs().mean(),
                      "sem_cls_acc": ep["last_sem_cls_scores"].detach().double().square().mean(),
                      "seed_ratio": ep["seed_features"].detach().float().mean(),
                      "quad_loss": 0.0,                                          # one of the reference's placeholders
                      "last_center": ep["last_center"].detach()}                 # not selected
        return bench.loss_of(ep)


def test_in_the_captured_step():
    """CapturedStep(stats=...) on the small procedural model with the optimiser and its schedule inside: over 6 steps with
    read() after step 3 and step 6 the sums are the per-step `.item()` sums taken on a twin stepper, bit for bit; building the
    stepper leaves an empty window; nothing is staged or re-uploaded during the replays"""
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(130 + i, 2, 8192, kind="room").to(dev) for i in range(6)]
    net, opt, sched = _model_and_optimizer(dev)
    crit = _Criterion()
    st = train_step.CapturedStep(net, crit, {"point_clouds": pcs[0]}, optimizer=opt, stats=lambda: crit.stats)
    assert st.launch == "hipGraph replay" and st.stats is not None
    assert sched.last_epoch == 0 and sched.get_last_lr() == [sched.lr_at(0, 2e-3), sched.lr_at(0, 1e-4)] and opt.t == 0
    empty = st.stats.read()
    assert (empty.steps, empty.calls) == (0, 0) and all(v == 0.0 for v in empty.values())
    assert list(empty) == ["center_abs_loss", "sem_cls_acc", "seed_ratio", "grad_norm", "quad_loss"]
    uploads, staged = st.stats.table_uploads, opt.staged

    net2, opt2, sched2 = _model_and_optimizer(dev)
    crit2 = _Criterion()
    st2 = train_step.CapturedStep(net2, crit2, {"point_clouds": pcs[0]}, optimizer=opt2)
    assert st2.stats is None

    sums, windows, wanted = {}, [], []
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        nx = None if nxt is None else {"point_clouds": nxt}
        st.step({"point_clouds": pc}, None, next_inputs=nx)
        st2.step({"point_clouds": pc}, None, next_inputs=nx)
        # the reference's loop on the twin: one synchronising read per key and step
        sums["grad_norm"] = opt2.grad_total_norm.item()
        for key, v in crit2.stats.items():
            if "loss" in key or "acc" in key or "ratio" in key:
                if key not in sums:
                    sums[key] = 0
                sums[key] += v if isinstance(v, float) else v.item()
        if i % 3 == 2:
            windows.append(st.stats.read())
            wanted.append(dict(sums))
            for key in sums:
                sums[key] = 0
    torch.cuda.synchronize()
    assert st.stats.table_uploads == uploads and opt.staged == staged and st.stats.copies == 3
    assert sched.last_epoch == sched2.last_epoch == 6 and sched.get_last_lr() == sched2.get_last_lr()
    for window, want in zip(windows, wanted):
        assert (window.steps, window.calls) == (3, 3) and set(window) == set(want)
        for key in want:
            assert _same(window[key], float(want[key])), (key, window[key], want[key])
        assert window["center_abs_loss"] > 0 and window["grad_norm"] > 0 and window["quad_loss"] == 0.0
    assert windows[0]["center_abs_loss"] != windows[1]["center_abs_loss"]
