"""Mean-teacher weight averaging inside FusedAdamW's finalise and update launches (optim.FusedAdamW.attach_teacher,
include/omnipq_optim.h: omnipq_adamw_ema_*) on the GPU, against the two-call route it replaces: FusedAdamW.step() followed by
ema.update_ema_variables(model, ema_model, decay, I).  The criterion is BIT equality: alpha and beta go through the same two
roundings on both routes (tests/test_fused_ema_host.py pins them) and an element is t = e * alpha, e = fmaf(beta, p_new, t) on
both.  One test does not lean on the other kernel: every teacher element against alpha * e + beta * p_new in float64.

The tensor set is tests/test_gpu_fused_adamw.py's: sizes 1, 3, 4095, 4096, 4097, 288 x 2048, 864 x 288 (head and tail peeling,
a chunk boundary, a short last chunk, many workgroups), views at element offsets 1, 2, 3 (mod 4) of one flat buffer, two
parameter groups, one parameter without a gradient (the ema_only workgroups).  The teacher's tensors are fresh allocations at
phase 0 -- so the views' teachers sit at ANOTHER phase than their partners and move through 4-byte-aligned accesses -- except the
teacher of the second view, which is a view at its partner's own phase (2 mod 4) and takes the 16-byte path behind a peeled head.
"""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_gpu_fused_adamw import (NAMES, SCALES, SIZES, VIEWS, attach, device_params, fused_opt, make_grads,  # noqa: E402
                                  start_values)

pytestmark = pytest.mark.gpu

COPHASED_TEACHER = 1                 # index into VIEWS: offset 5002 = 2 (mod 4), 4097 elements
_TEACHER_VALUES = None


class Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


def teacher_values():
    """CPU f32 start values of the teacher, one per parameter: values of their own, not a copy of the student's"""
    global _TEACHER_VALUES
    if _TEACHER_VALUES is None:
        g = torch.Generator().manual_seed(77)
        shapes = SIZES + [(n,) for _, n in VIEWS] + [(100,)]
        _TEACHER_VALUES = [torch.randn(s, generator=g) for s in shapes]
    return _TEACHER_VALUES


def make_pair(dev):
    """-> (student parameters, student module, teacher module); the teacher does not require gradients"""
    vals, flat = start_values()
    params = device_params(vals, flat, dev)
    tparams = []
    for i, (p, tv) in enumerate(zip(params, teacher_values())):
        if i - len(SIZES) == COPHASED_TEACHER:
            phase = (p.data_ptr() // 4) % 4
            buf = torch.zeros(tv.numel() + 8, device=dev)
            t = buf[phase:phase + tv.numel()]
            t.copy_(tv)
            assert (t.data_ptr() // 4) % 4 == phase == 2
        else:
            t = tv.to(dev)
            assert t.data_ptr() % 16 == 0
        tparams.append(torch.nn.Parameter(t, requires_grad=False))
    for v in range(len(VIEWS)):
        p, t = params[len(SIZES) + v], tparams[len(SIZES) + v]
        assert (p.data_ptr() % 16 == t.data_ptr() % 16) == (v == COPHASED_TEACHER)
    return params, Holder(params), Holder(tparams)


def assert_same(a, b, what):
    """parameters, both moments and every teacher tensor of two (params, opt, teacher) triples, bit for bit"""
    (pa, oa, ta), (pb, ob, tb) = a, b
    for name, p, q in zip(NAMES, pa, pb):
        assert torch.equal(p, q), (what, "parameter", name)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq), (what, "moments")
    for name, p, q in zip(NAMES, ta.parameters(), tb.parameters()):
        assert torch.equal(p, q), (what, "teacher", name)


def test_bit_equal_to_step_followed_by_update_ema_variables():
    """1: five steps at decay 0.75 -- 1 - 1/(I+1) = 0.5, 0.667, 0.75, 0.8, 0.833: both branches of the min and the tie at I = 3"""
    import ema
    dev = torch.device("cuda", 0)
    pa, ma, ta = make_pair(dev)
    pb, mb, tb = make_pair(dev)
    oa, ob = fused_opt(pa), fused_opt(pb)
    ob.attach_teacher(mb, tb, 0.75)
    assert ob.global_step == 1
    t_start = [t.detach().clone() for t in tb.parameters()]
    ka = kb = None
    alphas = []
    for i, scale in enumerate(SCALES):
        grads = make_grads(i, scale)
        ka, kb = attach(pa, grads, dev, ka), attach(pb, grads, dev, kb)
        na = oa.step().clone()
        alphas.append(ema.update_ema_variables(ma, ta, 0.75, i + 1))
        nb = ob.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(na, nb)
        assert_same((pa, oa, ta), (pb, ob, tb), f"step {i + 1}")
        assert ob.ema_coef.tolist() == [float(np.float32(alphas[-1])), float(np.float32(1.0 - alphas[-1]))]
    assert alphas == [0.5, 1.0 - 1.0 / 3.0, 0.75, 0.75, 0.75]
    assert ob.global_step == 6 and ob.t == 5 and ob.skipped == 0 and ob.table_builds == 1
    for name, t, t0 in zip(NAMES, tb.parameters(), t_start):                # every teacher moved, the no-gradient one too
        assert not torch.equal(t, t0), name
    # detach_teacher(): today's launches again -- the teacher stays, the students keep stepping alike
    ob.detach_teacher()
    frozen = [t.detach().clone() for t in tb.parameters()]
    grads = make_grads(9, 3e-4)
    attach(pa, grads, dev, ka), attach(pb, grads, dev, kb)
    oa.step(), ob.step()
    torch.cuda.synchronize()
    for name, p, q in zip(NAMES, pa, pb):
        assert torch.equal(p, q), name
    for t, t0 in zip(tb.parameters(), frozen):
        assert torch.equal(t, t0)


def test_every_teacher_element_against_float64():
    """2: one step from global_step = 4 (alpha = 0.8 under a decay of 0.999).  |e_new - (alpha * e + beta * p_new)| <=
    2^-23 * (|alpha * e| + |beta * p_new|) for EVERY element, the right-hand side in float64 from the f32 coefficients and the
    f32 p_new the kernel stored: two roundings of 2^-24 relative each, on e * alpha and on the fused multiply-add."""
    dev = torch.device("cuda", 0)
    params, model, teacher = make_pair(dev)
    opt = fused_opt(params)
    opt.attach_teacher(model, teacher, 0.999, global_step=4)
    e0 = [t.detach().double().cpu() for t in teacher.parameters()]
    p0 = [p.detach().clone() for p in params]
    attach(params, make_grads(0, 3e-4), dev)
    opt.step()
    torch.cuda.synchronize()
    a = np.fmin(1.0 - 1.0 / np.float64(4 + 1), np.float64(0.999))
    alpha, beta = np.float32(a), np.float32(1.0 - a)
    assert opt.ema_coef.tolist() == [float(alpha), float(beta)] and opt.global_step == 5
    assert torch.equal(params[-1], p0[-1]) and not torch.equal(params[0], p0[0])
    worst = 0.0
    for name, t, e, p in zip(NAMES, teacher.parameters(), e0, params):
        pn = p.detach().double().cpu()
        want = float(alpha) * e + float(beta) * pn
        bound = 2.0 ** -23 * ((float(alpha) * e).abs() + (float(beta) * pn).abs())
        err = (t.detach().double().cpu() - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        print(f"{name:<12} max err / bound = {ratio:.3f} over {err.numel()} elements")
        assert bool((err <= bound).all()), (name, ratio)
    print(f"worst err / bound = {worst:.3f}")


def test_accumulation_averages_on_applying_calls_only():
    """3: accum_steps = 3, seven calls: the teacher is bit-unchanged after calls 1, 2, 4, 5 and 7, and after calls 3 and 6 it is
    the twin's, which averages only when is_update_step"""
    import ema
    dev = torch.device("cuda", 0)
    pa, ma, ta = make_pair(dev)
    pb, mb, tb = make_pair(dev)
    oa, ob = fused_opt(pa, accum_steps=3), fused_opt(pb, accum_steps=3)
    ob.attach_teacher(mb, tb, 0.75)
    ka = kb = None
    step = 1
    for call in range(1, 8):
        grads = make_grads(40 + call, 2e-4)
        ka, kb = attach(pa, grads, dev, ka), attach(pb, grads, dev, kb)
        before = [t.detach().clone() for t in tb.parameters()]
        oa.step()
        if oa.is_update_step:
            ema.update_ema_variables(ma, ta, 0.75, step)
            step += 1
        ob.step()
        torch.cuda.synchronize()
        assert ob.is_update_step is (call in (3, 6))
        changed = [not torch.equal(t, t0) for t, t0 in zip(tb.parameters(), before)]
        if call in (3, 6):
            assert all(changed), (call, changed)
        else:
            assert not any(changed), (call, changed)
        assert_same((pa, oa, ta), (pb, ob, tb), f"call {call}")
    assert ob.global_step == 3 and ob.t == 2 and ob.micro == 1


def test_a_step_skipped_for_a_non_finite_gradient_still_averages():
    """4: inf in one gradient element on step 2 of 3 (a value, not a fault): parameters and moments stay, the teacher is
    averaged with the unchanged parameters as the twin's update_ema_variables does, and the step count goes on"""
    import ema
    dev = torch.device("cuda", 0)
    pa, ma, ta = make_pair(dev)
    pb, mb, tb = make_pair(dev)
    oa, ob = fused_opt(pa), fused_opt(pb)
    ob.attach_teacher(mb, tb, 0.75)
    ka = kb = None
    for i in range(3):
        grads = make_grads(50 + i, 3e-4)
        if i == 1:
            grads[5][17, 33] = float("inf")
        ka, kb = attach(pa, grads, dev, ka), attach(pb, grads, dev, kb)
        before = [p.detach().clone() for p in pb], ob.exp_avg.clone(), ob.exp_avg_sq.clone()
        t_before = [t.detach().clone() for t in tb.parameters()]
        oa.step()
        ema.update_ema_variables(ma, ta, 0.75, i + 1)
        norm = ob.step()
        torch.cuda.synchronize()
        if i == 1:
            assert not math.isfinite(float(norm)) and ob.skipped == 1 and ob.t == 1
            for p, q in zip(pb, before[0]):
                assert torch.equal(p, q)
            assert torch.equal(ob.exp_avg, before[1]) and torch.equal(ob.exp_avg_sq, before[2])
            assert all(not torch.equal(t, t0) for t, t0 in zip(tb.parameters(), t_before))
        assert_same((pa, oa, ta), (pb, ob, tb), f"step {i + 1}")
    assert ob.global_step == 4 and ob.t == 2 and ob.skipped == 1


def test_a_captured_launch_takes_the_alpha_of_its_own_step():
    """5: launch() under torch.cuda.graph after one eager step, replayed five times from global_step = 0, learning rate and decay
    changed between replays: bit-equal to an eager twin given the same values.  After the first replay (alpha = 0) the teacher
    IS the student, after the second it is not -- what a captured host-side alpha (0 for ever) could not do."""
    dev = torch.device("cuda", 0)
    pa, ma, ta = make_pair(dev)
    pb, mb, tb = make_pair(dev)
    oa, ob = fused_opt(pa), fused_opt(pb)
    oa.attach_teacher(ma, ta, 0.75)
    ob.attach_teacher(mb, tb, 0.75)
    grads = make_grads(60, 3e-4)
    ka, kb = attach(pa, grads, dev), attach(pb, grads, dev)
    oa.step(), ob.step()
    oa.set_global_step(0), ob.set_global_step(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.launch()
    builds = ob.table_builds
    lr0 = [g["lr"] for g in ob.param_groups]
    for i, (scale, decay) in enumerate(zip((1.0, 0.5, 0.5, 0.25, 2.0), (0.75, 0.75, 0.6, 0.6, 0.9))):
        grads = make_grads(61 + i, 3e-4)
        attach(pa, grads, dev, ka), attach(pb, grads, dev, kb)
        for opt in (oa, ob):
            for g, lr in zip(opt.param_groups, lr0):
                g["lr"] = lr * scale
            opt.ema_decay = decay
        oa.step()
        ob.sync_hyperparameters()
        graph.replay()
        torch.cuda.synchronize()
        assert_same((pa, oa, ta), (pb, ob, tb), f"replay {i + 1}")
        same = [torch.equal(t, p) for t, p in zip(tb.parameters(), pb)]
        if i == 0:
            assert all(same), same
        if i == 1:
            # (the parameter without a gradient has not moved since: its average with itself is itself)
            assert not any(same[:-1]) and same[-1], same
        want = min(1.0 - 1.0 / (i + 1), decay)
        assert ob.ema_coef.tolist() == [float(np.float32(want)), float(np.float32(1.0 - want))], i
    assert ob.global_step == oa.global_step == 5 and ob.t == oa.t == 6 and ob.table_builds == builds


def _model_teacher_optimizer(dev, accum_steps):
    from test_gpu_grad_accum import _model_and_optimizer
    net, opt = _model_and_optimizer(dev, accum_steps)
    teacher = copy.deepcopy(net)
    for p in teacher.parameters():
        p.requires_grad_(False)
    return net, teacher, opt


@pytest.mark.parametrize("step_freq", [1, 2])
def test_in_the_captured_step(step_freq):
    """6: CapturedStep(ema_in_step=True) on the small procedural model, four batches, against a twin stepper on the
    update_teacher(I) protocol; the criterion reads the teacher's outputs, so the student's weights also say that the teacher's
    forward saw the weights of BEFORE the averaging.  Building the stepper leaves the teacher and the global step alone."""
    sys.path.insert(0, REPO)
    import bench
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(90 + i, 2, 8192, kind="room").to(dev) for i in range(4)]

    def criterion(ep, labels, teacher_ep):
        return bench.loss_of(ep) + 0.1 * (ep["last_center"].float() - teacher_ep["last_center"].float()).square().mean()

    net, teacher, opt = _model_teacher_optimizer(dev, step_freq)
    names = [n for n, _ in net.named_parameters()]
    p0 = [p.detach().clone() for p in net.parameters()]
    t0 = [p.detach().clone() for p in teacher.parameters()]
    st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, teacher=teacher, ema=0.999,
                                 teacher_to_criterion=True, optimizer=opt, step_freq=step_freq, ema_in_step=True)
    assert st.launch == "hipGraph replay"
    for n, p, q in zip(names, net.parameters(), p0):
        assert torch.equal(p, q), n
    for n, p, q in zip(names, teacher.parameters(), t0):
        assert torch.equal(p, q), n
    assert opt.global_step == 1 and opt.t == 0 and opt.micro == 0
    with pytest.raises(RuntimeError, match="ema_in_step"):
        st.update_teacher(1)

    net2, teacher2, opt2 = _model_teacher_optimizer(dev, step_freq)
    st2 = train_step.CapturedStep(net2, criterion, {"point_clouds": pcs[0]}, teacher=teacher2, ema=0.999,
                                  teacher_to_criterion=True, optimizer=opt2, step_freq=step_freq)
    step = 1
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        nx = None if nxt is None else {"point_clouds": nxt}
        loss = st.step({"point_clouds": pc}, None, next_inputs=nx)
        assert torch.isfinite(loss).item()
        st2.step({"point_clouds": pc}, None, next_inputs=nx)
        if st2.is_update_step:
            st2.update_teacher(step)
            step += 1
        torch.cuda.synchronize()
        assert st.is_update_step == st2.is_update_step
        for n, p, q in zip(names, net.parameters(), net2.parameters()):
            assert torch.equal(p, q), (i, "student", n)
        for n, p, q in zip(names, teacher.parameters(), teacher2.parameters()):
            assert torch.equal(p, q), (i, "teacher", n)
    applied = 4 // step_freq
    assert opt.global_step == 1 + applied and opt.t == opt2.t == applied and opt.skipped == 0 and st.replays == 4
    assert any(not torch.equal(p, q) for p, q in zip(teacher.parameters(), t0))
