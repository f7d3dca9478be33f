"""Dynamic fp16 loss scaling on the GPU: optim.FusedAdamW(loss_scaler=...) (include/omnipq_optim.h:
omnipq_adamw_scaled_finalize) against the float64 restatement of tests/loss_scale_restatement.py -- which
tests/test_loss_scale_host.py holds to torch itself without a GPU -- next to torch.amp.GradScaler("cuda") + clip_grad_norm_ +
torch.optim.AdamW on the same scaled gradients; a scale held constant against the static route it must then equal bit for
bit (plain, accumulating, teacher attached); accumulation windows; the captured step and fp16 end to end.

Scale, growth tracker, step count and skip count are compared for EQUALITY after every step.  Parameters and moments are held
to the bound of test_gpu_fused_adamw.py (err_new <= 2 * err_torch + floor * 2^-23 * max|x| against the float64 truth, floor 1
for parameters and 4 for moments), the returned norm to one f32 rounding of the restatement's.
"""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, HERE)
import loss_scale_restatement as R  # noqa: E402
from test_gpu_fused_adamw import (BETAS, EPS, LRS, MAX_NORM, NAMES, ULP, WD, attach, device_params, fused_opt,  # noqa: E402
                                  groups_of, make_grads, max_err, moments, start_values)
from test_gpu_fused_ema import assert_same, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu

NEVER = 2 ** 31 - 1                  # a growth_interval no test reaches: the scale only ever backs off
S14 = 2.0 ** 14


def scaler(init=R.INIT, interval=R.INTERVAL):
    import optim
    return optim.LossScaler(init_scale=init, growth_factor=R.GROWTH, backoff_factor=R.BACKOFF, growth_interval=interval)


@pytest.mark.parametrize("init,schedule", [(R.INIT, R.SCHEDULE), (R.TOP, R.TOP_SCHEDULE)], ids=["every_branch", "growth_refused"])
def test_schedule_against_the_restatement_next_to_torchs_grad_scaler(init, schedule):
    """4"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    truth = R.ScaledTruth(vals, init_scale=init)
    params = device_params(vals, flat, dev)
    opt = fused_opt(params, loss_scaler=scaler(init))
    tparams = [torch.nn.Parameter(v.to(dev)) for v in vals]
    topt = torch.optim.AdamW(groups_of(tparams), lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    witness = torch.amp.GradScaler("cuda", init_scale=init, growth_factor=R.GROWTH, backoff_factor=R.BACKOFF,
                                   growth_interval=R.INTERVAL)
    witness.scale(torch.zeros(1, device=dev))                        # GradScaler creates its two tensors lazily
    assert opt.scale_value == truth.scale == init and opt.growth_tracker == 0
    keep, trajectory = None, []
    for kind, grads in zip(schedule, R.unscaled_grads(schedule)):
        sg = R.scaled(grads, truth.scale, kind)
        keep = attach(params, sg, dev, keep)
        before = [p.detach().clone() for p in params], opt.exp_avg.clone(), opt.exp_avg_sq.clone()
        got = float(opt.step())
        norm, ok = truth.step(sg)
        state = (opt.scale_value, opt.growth_tracker, opt.t, opt.skipped)
        print(f"{kind:>6}: norm {got:.9g} (restated {norm:.9g})  scale, tracker, t, skipped = {state}")
        assert state == (truth.scale, truth.tracker, truth.t, truth.skipped), (kind, state)
        trajectory.append(state[0] / init)
        if ok:
            assert abs(got - norm) <= ULP * norm, (got, norm)
        else:                                                        # a skipped step leaves p, m and v bit-unchanged
            assert not math.isfinite(got) and not math.isfinite(norm)
            for name, p, q in zip(NAMES, params, before[0]):
                assert torch.equal(p, q), name
            assert torch.equal(opt.exp_avg, before[1]) and torch.equal(opt.exp_avg_sq, before[2])
        # the second witness: torch's own scaler and optimiser on the device, same scaled gradients
        for p, g in zip(tparams, sg):
            p.grad = None if g is None else g.to(dev)
        witness.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM, foreach=False)
        witness.step(topt)
        witness.update()
        assert (witness.get_scale(), witness._get_growth_tracker()) == state[:2], kind
    assert float(topt.state[tparams[0]]["step"]) == opt.t
    if schedule is R.SCHEDULE:
        assert trajectory == [1, 1, 2, 1, 1, 0.5, 0.5, 0.5, 1] and opt.t == 7 and opt.skipped == 2
    else:
        assert trajectory == [1, 1, 1] and opt.growth_tracker == 0 and opt.t == 3
    mom, failures = moments(opt, params), []
    for i, name in enumerate(NAMES[:-1]):
        tst = topt.state[tparams[i]]
        for what, new, old, want, floor in (("param", params[i], tparams[i], truth.p[i], 1.0),
                                            ("exp_avg", mom[i][0], tst["exp_avg"], truth.m[i], 4.0),
                                            ("exp_avg_sq", mom[i][1], tst["exp_avg_sq"], truth.v[i], 4.0)):
            e_new, e_old, big = max_err(new, want), max_err(old, want), float(want.abs().max())
            bound = 2 * e_old + floor * ULP * big
            line = f"  {name:<14}{what:<12}{e_new:>12.3e}{e_old:>12.3e}{bound:>12.3e}  {big:.3e}"
            print(line)
            if not e_new <= bound:
                failures.append(line)
    assert not failures, "\n".join(failures)
    assert torch.equal(params[-1].detach().cpu(), vals[-1])


_LOG_UNIFORM = None


def log_uniform_steps():
    """the gradients of the existing static-scale test (magnitudes in [1e-6, 1e2]: times 2^14 nothing leaves f32's normal
    range, so the scaling is exact), computed once"""
    global _LOG_UNIFORM
    if _LOG_UNIFORM is None:
        steps = [make_grads(i, None, log_uniform=True) for i in range(3)]
        for g in steps[0][:-1]:
            assert 9.9e-7 <= float(g.abs().min()) and float(g.abs().max()) <= 1.01e2
        _LOG_UNIFORM = [[None if g is None else g * S14 for g in grads] for grads in steps]
    return _LOG_UNIFORM


@pytest.mark.parametrize("family", ["plain", "accum", "teacher"])
def test_a_scale_held_constant_is_the_static_route_bit_for_bit(family):
    """5: growth_interval out of reach, init_scale 2^14: parameters, moments, the teacher and every returned norm equal
    FusedAdamW(grad_scale = 2^-14 x the user's) on the same scaled gradients -- the squared-norm and update launches see the
    scale through result[3] only"""
    dev = torch.device("cuda", 0)
    steps = log_uniform_steps()
    kw = dict(accum_steps=3) if family == "accum" else {}
    user = 1.0 / 3.0 if family == "accum" else 1.0
    calls = steps + steps[::-1] if family == "accum" else steps                  # two windows of three micro-batches
    runs = []
    for dynamic in (False, True):
        params, student, teacher = make_pair(dev)
        if dynamic:
            opt = fused_opt(params, grad_scale=user, loss_scaler=scaler(S14, NEVER), **kw)
        else:
            opt = fused_opt(params, grad_scale=user * 2.0 ** -14, **kw)
        if family == "teacher":
            opt.attach_teacher(student, teacher, 0.75)
        keep, norms = None, []
        for grads in calls:
            keep = attach(params, grads, dev, keep)
            norms.append(opt.step().clone())
        torch.cuda.synchronize()
        runs.append((params, opt, teacher, norms))
    a, b = runs
    assert a[1].t == b[1].t == (2 if family == "accum" else 3) and b[1].skipped == 0
    assert float(b[1].result[1]) < 1.0                             # clipped: the coefficient is part of what must agree
    assert b[1].scale_value == S14 and b[1].growth_tracker == b[1].t
    assert_same(a[:3], b[:3], family)
    assert torch.equal(a[1].result, b[1].result)
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert torch.equal(x, y), (family, "norm of call", i, float(x), float(y))
    if family == "teacher":
        assert a[1].global_step == b[1].global_step == 4
    else:                                                          # (the unattached teacher is the untouched start)
        assert a[1].global_step is None


def test_accumulation_backs_off_once_per_window_on_the_applying_call():
    """6: k = 3, a non-finite value in the MIDDLE micro-batch: the scale stays through calls 1 and 2 and is halved by call 3,
    which skips and still averages the teacher; the next window equals a fresh optimiser started at the halved scale"""
    dev = torch.device("cuda", 0)
    pa, ma, ta = make_pair(dev)
    oa = fused_opt(pa, accum_steps=3, grad_scale=1.0 / 3.0, loss_scaler=scaler(S14, 2))
    oa.attach_teacher(ma, ta, 0.75)
    p0 = [p.detach().clone() for p in pa]
    keep = None
    for j in range(3):
        grads = R.scaled(make_grads(60 + j, 2e-4), S14, "inf" if j == 1 else "finite")
        keep = attach(pa, grads, dev, keep)
        t_before = [t.detach().clone() for t in ta.parameters()]
        norm = float(oa.step())
        changed = [not torch.equal(t, t0) for t, t0 in zip(ta.parameters(), t_before)]
        assert math.isfinite(norm) == (j == 0)                    # the running sum keeps the inf
        if j < 2:
            assert (oa.scale_value, oa.growth_tracker, oa.skipped, oa.is_update_step) == (S14, 0, 0, False), j
            assert not any(changed), j
        else:
            assert (oa.scale_value, oa.growth_tracker, oa.skipped, oa.t, oa.is_update_step) == (S14 / 2, 0, 1, 0, True)
            assert all(changed)                                    # the skipped window still averaged the teacher
    for name, p, q in zip(NAMES, pa, p0):
        assert torch.equal(p, q), name
    assert not oa.exp_avg.any().item() and not oa.exp_avg_sq.any().item() and oa.global_step == 2
    # a fresh optimiser at the backed-off scale, its teacher where the skipped window's averaging left this one's
    pb, mb, tb = make_pair(dev)
    with torch.no_grad():
        for t, s in zip(tb.parameters(), ta.parameters()):
            t.copy_(s)
    ob = fused_opt(pb, accum_steps=3, grad_scale=1.0 / 3.0, loss_scaler=scaler(S14 / 2, 2))
    ob.attach_teacher(mb, tb, 0.75, global_step=2)
    kb = None
    for j in range(3):
        grads = R.scaled(make_grads(70 + j, 2e-4), S14 / 2)
        keep, kb = attach(pa, grads, dev, keep), attach(pb, grads, dev, kb)
        na, nb = oa.step().clone(), ob.step().clone()
        assert torch.equal(na, nb) and math.isfinite(float(na)), j
    torch.cuda.synchronize()
    assert_same((pa, oa, ta), (pb, ob, tb), "the window after the skipped one")
    assert (oa.scale_value, oa.growth_tracker, oa.t, oa.skipped) == (S14 / 2, 1, 1, 1)
    assert (ob.scale_value, ob.growth_tracker, ob.t, ob.skipped) == (S14 / 2, 1, 1, 0)
    assert any(not torch.equal(p, q) for p, q in zip(pa, p0))


def _model_and_optimizer(dev, loss_scaler):
    """the model and the two parameter groups of test_gpu_fused_adamw.py::test_in_the_captured_step"""
    sys.path.insert(0, REPO)
    import bench
    import optim
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    net = load_procedural(bench.build_model(0)).to(dev).train()
    zero_dropout(net)
    groups = [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
              {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": LRS[1]}]
    return net, optim.FusedAdamW(groups, lr=LRS[0], weight_decay=WD, max_norm=MAX_NORM, loss_scaler=loss_scaler)


def test_in_the_captured_step():
    """7: seven replays with growth_interval = 2; the criterion multiplies its loss by a device scalar the test sets to inf
    in front of replays 3 and 4 (NaN arithmetic in ordinary kernels: values, not a fault)"""
    import bench
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(90 + i % 3, 2, 8192, kind="room").to(dev) for i in range(7)]
    poison = torch.ones((), device=dev)

    def criterion(ep, labels):
        return bench.loss_of(ep) * poison                          # no host read: the replay follows the device word

    init = 2.0 ** 10
    net, opt = _model_and_optimizer(dev, scaler(init, 2))
    st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, optimizer=opt, loss_scale="dynamic")
    assert st.launch == "hipGraph replay"
    assert (opt.scale_value, opt.growth_tracker, opt.t, opt.skipped) == (init, 0, 0, 0)      # building left no trace
    assert not opt.exp_avg.any().item()
    want = [(1, 1), (2, 0), (1, 0), (0.5, 0), (0.5, 1), (1, 0), (1, 1)]        # init -> x2 -> x1/2 -> x1/2 -> x2
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        bad = i in (2, 3)
        poison.fill_(float("inf") if bad else 1.0)
        before = [p.detach().clone() for p in net.parameters()]
        loss = st.step({"point_clouds": pc}, None, next_inputs=None if nxt is None else {"point_clouds": nxt})
        torch.cuda.synchronize()
        got = (opt.scale_value / init, opt.growth_tracker)
        print(f"replay {i + 1}: loss {float(loss.detach()):.6g} norm {float(st.grad_total_norm):.6g} scale, tracker = {got}")
        assert got == want[i], (i, got)
        same = [torch.equal(p, q) for p, q in zip(net.parameters(), before)]
        if bad:
            assert all(same) and not math.isfinite(float(st.grad_total_norm)), i
        else:
            assert not all(same) and math.isfinite(float(loss.detach())) and math.isfinite(float(st.grad_total_norm)), i
    assert st.replays == 7 and opt.t == 5 and opt.skipped == 2 and opt.t + opt.skipped == 7


def test_fp16_end_to_end():
    """8: amp_dtype = float16 with the default scaler (2^16) and growth out of reach.  Whether a step overflows is not
    predicted: the bookkeeping must hold either way"""
    import _ext
    import bench
    import synth
    import train_step
    assert _ext.E16.available(torch.float16), "the IEEE-half library is part of every build"
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(90 + i % 3, 2, 8192, kind="room").to(dev) for i in range(4)]
    net, opt = _model_and_optimizer(dev, scaler(R.INIT, NEVER))
    st = train_step.CapturedStep(net, lambda ep, labels: bench.loss_of(ep), {"point_clouds": pcs[0]}, optimizer=opt,
                                 loss_scale="dynamic", amp_dtype=torch.float16)
    assert st.launch == "hipGraph replay" and (opt.scale_value, opt.growth_tracker, opt.t, opt.skipped) == (R.INIT, 0, 0, 0)
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        loss = st.step({"point_clouds": pc}, None, next_inputs=None if nxt is None else {"point_clouds": nxt})
        print(f"replay {i + 1}: loss {float(loss.detach()):.6g} norm {float(st.grad_total_norm):.6g} scale {opt.scale_value:g} "
              f"skipped {opt.skipped}")
        assert math.isfinite(float(loss.detach())), i
    assert opt.t + opt.skipped == 4
    assert opt.scale_value == 2.0 ** 16 * 0.5 ** opt.skipped and opt.growth_tracker <= opt.t
