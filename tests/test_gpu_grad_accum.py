"""Gradient accumulation on the GPU: optim.FusedAdamW(accum_steps=k) (include/omnipq_optim.h: omnipq_adamw_accum_*) against an
accum_steps=1 FusedAdamW stepped on the gradients torch summed in f32, (g1 + g2) + g3, on the device -- and
train_step.CapturedStep(step_freq=2) against a stepper without optimiser whose gradients are summed from the host.

Every criterion is BIT equality: the accumulator is one f32 add per element in the order the micro-batches arrive, the norm
pass squares the running sum in the summation order of omnipq_adamw_grad_sqnorm on a gradient at the same address, and the
update reads the accumulator where it read the gradient.  There is nothing to tolerate.

The tensor set is tests/test_gpu_fused_adamw.py's: sizes 1, 3, 4095, 4096, 4097, 288 x 2048, 864 x 288, views at element offsets
1, 2, 3 (mod 4) of which one is not co-phased with its gradient, one parameter without a gradient.
"""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_gpu_fused_adamw import (FLAT, LRS, MAX_NORM, NAMES, SIZES, VIEWS, WD, attach, device_params, fused_opt,  # noqa: E402
                                  make_grads, start_values)

pytestmark = pytest.mark.gpu


def summed(dev, sets):
    """((g1 + g2) + g3) ... per parameter, f32 adds by torch on the device"""
    out = []
    for per_param in zip(*sets):
        if per_param[0] is None:
            out.append(None)
            continue
        s = per_param[0].to(dev)
        for g in per_param[1:]:
            s = s + g.to(dev)
        out.append(s)
    return out


def state_of(params, opt):
    return [p.detach().clone() for p in params], opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def assert_same_state(params, opt, want_params, want_opt, what):
    for name, p, q in zip(NAMES, params, want_params):
        assert torch.equal(p, q), (what, name)
    assert torch.equal(opt.exp_avg, want_opt.exp_avg), what
    assert torch.equal(opt.exp_avg_sq, want_opt.exp_avg_sq), what


def assert_unchanged(params, opt, before, what):
    ps, m, v = before
    for name, p, q in zip(NAMES, params, ps):
        assert torch.equal(p, q), (what, name)
    assert torch.equal(opt.exp_avg, m) and torch.equal(opt.exp_avg_sq, v), what


def macro_step(dev, params, opt, sets, keep=None):
    """one call per micro-batch -> (the norm each call returned, the gradient tensors)"""
    norms = []
    for grads in sets:
        keep = attach(params, grads, dev, keep)
        norms.append(opt.step().clone())
    return norms, keep


def reference_step(dev, params, opt, sets, keep=None):
    """an accum_steps=1 optimiser on the sum of the micro-batches' gradients"""
    keep = attach(params, summed(dev, sets), dev, keep)
    return opt.step().clone(), keep


# one macro-step of norm ~ 1.6 (clipped at max_norm = 0.1) and one of norm ~ 0.03 (not clipped)
MACRO = [[make_grads(10 + i, 1e-3) for i in range(3)], [make_grads(20 + i, 2e-5) for i in range(3)]]


def test_three_micro_batches_are_one_step_on_their_sum():
    """1: accum_steps=3, two macro-steps; after each applying call parameters, moments, norm and t are those of the
    accum_steps=1 optimiser on the summed gradients, after each other call nothing has moved"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    params = device_params(vals, flat, dev)
    opt = fused_opt(params, accum_steps=3)
    rparams = device_params(vals, flat, dev)
    ropt = fused_opt(rparams)
    keep = rkeep = None
    clipped = []
    for n, sets in enumerate(MACRO):
        for i, grads in enumerate(sets):
            before = state_of(params, opt)
            keep = attach(params, grads, dev, keep)
            norm = opt.step().clone()
            assert opt.micro == (i + 1) % 3 and opt.is_update_step is (i == 2)
            assert int(opt.accum[0]) == opt.micro                       # the host mirror is the device word
            if i < 2:
                assert_unchanged(params, opt, before, (n, i))
                assert opt.t == n and opt.skipped == 0
                # the norm of the running sum so far, within one rounding to f32 of its float64 value
                want = math.sqrt(sum(float(s.double().square().sum()) for s in summed(dev, sets[:i + 1]) if s is not None))
                assert abs(float(norm) - want) <= 2.0 ** -23 * want, (n, i, float(norm), want)
        rnorm, rkeep = reference_step(dev, rparams, ropt, sets, rkeep)
        torch.cuda.synchronize()
        assert_same_state(params, opt, rparams, ropt, f"macro-step {n}")
        assert torch.equal(norm, rnorm), (n, float(norm), float(rnorm))
        assert torch.equal(opt.result, ropt.result), n                  # clip coefficient, flag, g coefficient as documented
        assert opt.t == ropt.t == n + 1 and opt.skipped == 0
        assert any(not torch.equal(p, q) for p, q in zip(params, before[0])), "the applying call did not move the weights"
        clipped.append(float(opt.result[1]) < 1.0)
    assert clipped == [True, False], clipped
    assert opt.table_builds == 1                                        # same gradient addresses: the table was built once
    # the parameter whose .grad is None: bit-unchanged, and so are its moments and its accumulator segment
    assert torch.equal(params[-1].detach().cpu(), vals[-1])
    o = opt._offset[params[-1]]
    assert not opt.exp_avg[o:o + 100].any().item() and not opt.exp_avg_sq[o:o + 100].any().item()
    assert not opt.acc[o:o + 100].any().item()
    # the views moved their slice of the flat buffer and nothing around it
    untouched = torch.ones(FLAT, dtype=torch.bool)
    for o, n in VIEWS:
        untouched[o:o + n] = False
    assert torch.equal(params[len(SIZES)].flat_buffer.cpu()[untouched], flat[untouched])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_micro_batch_skips_the_macro_step(bad):
    """2: a non-finite value in the MIDDLE micro-batch: the applying call changes nothing and counts as skipped; the next
    macro-step overwrites the accumulator and equals the same macro-step on a fresh optimiser"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    params = device_params(vals, flat, dev)
    opt = fused_opt(params, accum_steps=3)
    before = state_of(params, opt)
    sets = [[None if g is None else g.clone() for g in grads] for grads in MACRO[1]]
    sets[1][5][17, 33] = bad
    sets[1][2][4094] = bad                                              # ... and in a peeled tail
    norms, keep = macro_step(dev, params, opt, sets)
    assert math.isfinite(float(norms[0])) and not math.isfinite(float(norms[1])) and not math.isfinite(float(norms[2]))
    assert opt.t == 0 and opt.skipped == 1 and opt.micro == 0 and int(opt.accum[0]) == 0
    assert_unchanged(params, opt, before, "skipped macro-step")
    assert not torch.isfinite(opt.acc).all().item()                     # the accumulator does hold what must not leak
    norms, _ = macro_step(dev, params, opt, MACRO[0], keep)
    fparams = device_params(vals, flat, dev)
    fopt = fused_opt(fparams, accum_steps=3)
    fnorms, _ = macro_step(dev, fparams, fopt, MACRO[0])
    torch.cuda.synchronize()
    assert_same_state(params, opt, fparams, fopt, "the macro-step after the skipped one")
    for x, y in zip(norms, fnorms):
        assert torch.equal(x, y) and math.isfinite(float(x))
    assert opt.t == fopt.t == 1 and opt.skipped == 1 and fopt.skipped == 0


def test_reset_accumulation_discards_the_partial_sum():
    """3: one micro-step, reset, a full macro-step == the macro-step alone"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    params = device_params(vals, flat, dev)
    opt = fused_opt(params, accum_steps=3)
    _, keep = macro_step(dev, params, opt, [make_grads(30, 1e-3)])
    assert opt.micro == 1
    opt.reset_accumulation()
    assert opt.micro == 0 and opt.is_update_step is False
    norms, _ = macro_step(dev, params, opt, MACRO[1], keep)
    fparams = device_params(vals, flat, dev)
    fopt = fused_opt(fparams, accum_steps=3)
    fnorms, _ = macro_step(dev, fparams, fopt, MACRO[1])
    torch.cuda.synchronize()
    assert_same_state(params, opt, fparams, fopt, "after reset_accumulation")
    for x, y in zip(norms, fnorms):
        assert torch.equal(x, y)
    assert opt.t == fopt.t == 1 and opt.micro == 0 and int(opt.accum[0]) == 0


def test_the_active_set_is_fixed_inside_an_accumulation_its_addresses_are_not():
    """4: at micro == 1 a parameter that loses (or gains) its gradient is refused; fresh gradient tensors are not"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    params = device_params(vals, flat, dev)
    opt = fused_opt(params, accum_steps=3)
    sets = MACRO[1]
    attach(params, sets[0], dev)
    opt.step()
    assert opt.micro == 1
    attach(params, sets[1], dev)                                        # new addresses ...
    g2 = params[2].grad
    params[2].grad = None                                               # ... and one parameter fewer
    with pytest.raises(RuntimeError, match="set of parameters with gradients changed"):
        opt.step()
    params[2].grad = g2
    params[-1].grad = torch.zeros_like(params[-1])                      # one parameter more
    with pytest.raises(RuntimeError, match="set of parameters with gradients changed"):
        opt.step()
    params[-1].grad = None
    assert opt.micro == 1 and int(opt.accum[0]) == 1 and opt.t == 0     # a refused call launched nothing
    norms = [opt.step().clone()]                                        # the same set at new addresses: legal
    attach(params, sets[2], dev)
    norms.append(opt.step().clone())
    assert opt.table_builds == 3 and opt.is_update_step
    fparams = device_params(vals, flat, dev)
    fopt = fused_opt(fparams, accum_steps=3)
    fnorms, _ = macro_step(dev, fparams, fopt, sets)
    torch.cuda.synchronize()
    assert fopt.table_builds == 1
    assert_same_state(params, opt, fparams, fopt, "fresh gradient tensors for every micro-batch")
    assert torch.equal(norms[0], fnorms[1]) and torch.equal(norms[1], fnorms[2])
    assert opt.t == fopt.t == 1


def _model_and_optimizer(dev, accum_steps):
    sys.path.insert(0, REPO)
    import bench
    import optim
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    net = load_procedural(bench.build_model(0)).to(dev).train()
    zero_dropout(net)
    groups = [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
              {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": LRS[1]}]
    opt = optim.FusedAdamW(groups, lr=LRS[0], weight_decay=WD, max_norm=MAX_NORM, accum_steps=accum_steps)
    return net, opt


def test_in_the_captured_step():
    """5: CapturedStep(step_freq=2) with the accumulating optimiser inside, four batches, against an identical model whose
    stepper has no optimiser: its gradients are cloned and summed after each replay and an accum_steps=1 FusedAdamW steps
    every second call.  A cosine schedule on both, stepped on applying steps only."""
    sys.path.insert(0, REPO)
    import bench
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(90 + i, 2, 8192, kind="room").to(dev) for i in range(4)]

    def criterion(ep, labels):
        return bench.loss_of(ep)

    net, opt = _model_and_optimizer(dev, 2)
    names = [n for n, _ in net.named_parameters()]
    p0 = [p.detach().clone() for p in net.parameters()]
    st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, optimizer=opt, step_freq=2)
    assert st.launch == "hipGraph replay"
    # building the stepper (three warm-up steps and the capture run: four calls of launch()) left no trace
    for n, p, q in zip(names, net.parameters(), p0):
        assert torch.equal(p, q), n
    assert not opt.exp_avg.any().item() and not opt.exp_avg_sq.any().item()
    assert opt.t == 0 and opt.skipped == 0
    assert opt.micro == 0 and opt.accum.tolist() == [0, 0] and st.is_update_step is False
    builds = opt.table_builds
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=2)

    net2, opt2 = _model_and_optimizer(dev, 1)
    for p, q in zip(net2.parameters(), p0):
        assert torch.equal(p, q)
    st2 = train_step.CapturedStep(net2, criterion, {"point_clouds": pcs[0]})
    sched2 = torch.optim.lr_scheduler.CosineAnnealingLR(opt2, T_max=2)

    flags, held = [], None
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        nx = None if nxt is None else {"point_clouds": nxt}
        before = [p.detach().clone() for p in net.parameters()]
        loss = st.step({"point_clouds": pc}, None, next_inputs=nx)
        flags.append(st.is_update_step)
        assert torch.isfinite(loss).item() and math.isfinite(float(st.grad_total_norm))
        st2.step({"point_clouds": pc}, None, next_inputs=nx)
        grads = [None if p.grad is None else p.grad.detach().clone() for p in net2.parameters()]
        if i % 2 == 0:
            held = grads
        else:
            for p, a, b in zip(net2.parameters(), held, grads):
                assert (a is None) == (b is None)
                p.grad = None if a is None else a + b
            norm2 = opt2.step().clone()
        torch.cuda.synchronize()
        for n, p, q in zip(names, net.parameters(), net2.parameters()):
            assert torch.equal(p, q), (i, n)
        moved = any(not torch.equal(p, q) for p, q in zip(net.parameters(), before))
        if i % 2 == 0:
            assert not moved, f"replay {i} is not an applying one and moved the weights"
            assert opt.micro == 1 and int(opt.accum[0]) == 1
        else:
            assert moved, f"replay {i} did not move the weights"
            assert torch.equal(st.grad_total_norm, norm2), (i, float(st.grad_total_norm), float(norm2))
            assert opt.micro == 0 and int(opt.accum[0]) == 0
            sched.step()
            sched2.step()
        assert opt.t == opt2.t == (i + 1) // 2 and opt.skipped == 0
    assert flags == [False, True, False, True]
    assert opt.t == 2 and st.replays == 4 and opt.table_builds == builds
    assert torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)
