"""omni-pq_amd/optim.py on the GPU: FusedAdamW (clip + AdamW in three HIP launches, include/omnipq_optim.h) against the same
recurrence in float64, next to torch.optim.AdamW(foreach=False) + clip_grad_norm_ in f32 on the same gradients; its norm,
run-to-run bits, the skip on non-finite gradients, the static loss scale, the captured step and checkpoints.

The parity bound (tests 1 and 6c), per tensor, max-abs against the float64 truth:

    err_new <= 2 * err_torch + 2^-23 * max|x|

-- two correct f32 evaluation orders differ by as much as either differs from the truth (torch's own foreach and fused paths
do), and the floor is one ulp of the tensor's largest element.  For the PARAMETERS that is the bound as stated; the moments go
through a chain of five roundings per step (g' = c * g, (1 - b) * g', * g', the fused multiply-add, and the clip coefficient's
own f32 rounding) where a parameter goes through two, so their floor is 4 * 2^-23 * max|x|.

Measured on MI355X (profiles/fused_adamw_parity.txt holds every tensor): the parameters' err_new equals err_torch to three
digits in 9 of 10 tensors (up to 2.1e-6 at max|p| = 4.4, five steps), no err_new above 0.45 x its bound, moments included;
the captured step's first update (519 tensors): worst err_new 0.66 x its bound.
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

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
LRS, WD, BETAS, EPS, MAX_NORM = (2e-3, 1e-4), 5e-4, (0.9, 0.999), 1e-8, 0.1
SIZES = [(1,), (3,), (4095,), (4096,), (4097,), (288, 2048), (864, 288)]
VIEWS = [(1, 5000), (5002, 4097), (9103, 9001)]          # (element offset, length) in one flat buffer: offsets = 1, 2, 3 mod 4
FLAT = 18112
COPHASED = (True, False, True)                           # does the view's gradient sit at the same offset of a flat gradient?
NAMES = [f"p{'x'.join(map(str, s))}" for s in SIZES] + [f"view+{o % 4}" for o, _ in VIEWS] + ["nograd"]
GROUP = [0, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0]                # parameter -> group


def start_values(seed=0):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=g) for s in SIZES]
    flat = torch.randn(FLAT, generator=g)
    vals += [flat[o:o + n].clone() for o, n in VIEWS]
    vals.append(torch.randn(100, generator=g))
    return vals, flat


def make_grads(seed, scale, log_uniform=False):
    """CPU f32 gradients for every parameter (None for the last one)"""
    g = torch.Generator().manual_seed(1000 + seed)
    shapes = SIZES + [(n,) for _, n in VIEWS]
    if log_uniform:      # magnitudes in [1e-6, 1e2]: the range in which scaling by 2^14 is exact in f32 (test 5)
        out = [(10.0 ** (torch.rand(s, generator=g) * 8 - 6)) * (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
               for s in shapes]
    else:
        out = [torch.randn(s, generator=g) * scale for s in shapes]
    return out + [None]


def device_params(vals, flat, dev):
    """the parameters on the GPU; the three views are Parameters INTO one flat buffer at offsets 1, 2, 3 (mod 4) elements"""
    dflat = flat.to(dev)
    params = [torch.nn.Parameter(v.to(dev)) for v in vals[:len(SIZES)]]
    params += [torch.nn.Parameter(dflat[o:o + n]) for o, n in VIEWS]
    params.append(torch.nn.Parameter(vals[-1].to(dev)))
    for p, (o, _) in zip(params[len(SIZES):], VIEWS):
        assert (p.data_ptr() // 4) % 4 == o % 4
    params[len(SIZES)].flat_buffer = dflat
    return params


def attach(params, grads, dev, keep=None):
    """p.grad = the step's gradients; the co-phased views take theirs from a flat gradient buffer at the view's own offset.
    keep: gradient tensors of an earlier call to refill in place (same addresses: the device table is not rebuilt)"""
    if keep is not None:
        for p, g, k in zip(params, grads, keep):
            if g is not None:
                k.copy_(g)
                p.grad = k
        return keep
    gflat = torch.zeros(FLAT, device=dev)
    out = []
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
            out.append(None)
            continue
        v = i - len(SIZES)
        if 0 <= v and COPHASED[v]:
            o, n = VIEWS[v]
            t = gflat[o:o + n]
            t.copy_(g)
        else:
            t = g.to(dev)
        p.grad = t
        out.append(t)
    return out


def groups_of(params, lrs=LRS):
    return [{"params": [p for p, gi in zip(params, GROUP) if gi == 0], "lr": lrs[0]},
            {"params": [p for p, gi in zip(params, GROUP) if gi == 1], "lr": lrs[1]}]


def fused_opt(params, **kw):
    import optim
    kw.setdefault("max_norm", MAX_NORM)
    return optim.FusedAdamW(groups_of(params), lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, **kw)


class Truth:
    """the recurrence of include/omnipq_optim.h in float64 on the CPU, from the same f32 start"""

    def __init__(self, vals, lrs=LRS, max_norm=MAX_NORM, grad_scale=1.0):
        self.p = [v.double().clone() for v in vals]
        self.m = [torch.zeros_like(v) for v in self.p]
        self.v = [torch.zeros_like(v) for v in self.p]
        self.t, self.lrs, self.max_norm, self.gs = 0, lrs, max_norm, grad_scale

    def step(self, grads, group=GROUP):
        sq = sum(float((self.gs * g.double()).square().sum()) for g in grads if g is not None)
        norm = math.sqrt(sq)
        clip = min(1.0, self.max_norm / (norm + 1e-6)) if self.max_norm > 0 else 1.0
        self.t += 1
        b1, b2 = BETAS
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for i, g in enumerate(grads):
            if g is None:
                continue
            lr = self.lrs[group[i]]
            gp = self.gs * clip * g.double()
            self.p[i] *= 1 - lr * WD
            self.m[i] = b1 * self.m[i] + (1 - b1) * gp
            self.v[i] = b2 * self.v[i] + (1 - b2) * gp * gp
            self.p[i] -= (lr / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + EPS)
        return norm, clip


def max_err(x, want):
    return float((x.detach().double().cpu() - want).abs().max())


SCALES = (1e-3, 5e-5, 1e-3, 2e-5, 3e-4)                  # gradient norms ~ 0.9, 0.046, 0.9, 0.018, 0.27 around max_norm = 0.1


def run_fused(dev, vals, flat, steps, **kw):
    params = device_params(vals, flat, dev)
    opt = fused_opt(params, **kw)
    norms, keep = [], None
    for grads in steps:
        keep = attach(params, grads, dev, keep)
        norms.append(opt.step().clone())
    torch.cuda.synchronize()
    return params, opt, norms


def moments(opt, params):
    return [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) if p in opt.state and "exp_avg" in opt.state[p] else None
            for p in params]


def test_arithmetic_against_float64_next_to_torch_adamw():
    """1 + 2: five steps, clipped and unclipped, every alignment; parameters and moments within the bound, the returned
    norm within 2^-23 relative of the float64 norm; the parameter without a gradient and its moments untouched."""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    steps = [make_grads(i, s) for i, s in enumerate(SCALES)]
    params, opt, norms = run_fused(dev, vals, flat, steps)
    assert opt.table_builds == 1                                   # same gradient addresses every step: built once
    # torch: foreach=False AdamW + clip_grad_norm_ in f32 on plain tensors holding the same values
    tparams = [torch.nn.Parameter(v.to(dev)) for v in vals]
    topt = torch.optim.AdamW(groups_of(tparams), lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    truth = Truth(vals)
    clipped = []
    for grads, got in zip(steps, norms):
        for p, g in zip(tparams, grads):
            p.grad = None if g is None else g.to(dev)
        torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM, foreach=False)
        topt.step()
        norm, clip = truth.step(grads)
        clipped.append(clip < 1.0)
        rel = abs(float(got) - norm) / norm
        print(f"norm {float(got):.9g} truth {norm:.17g} rel {rel:.3e} clip {clip:.6f}")
        assert rel <= ULP, (float(got), norm, rel)
    assert any(clipped) and not all(clipped), clipped
    assert opt.t == 5 and opt.skipped == 0
    mom = moments(opt, params)
    lines = ["# tests/test_gpu_fused_adamw.py::test_arithmetic_against_float64_next_to_torch_adamw: max-abs error against the",
             "# float64 recurrence after five steps; new = FusedAdamW, torch = torch.optim.AdamW(foreach=False) + clip_grad_norm_",
             f"# {'tensor':<14}{'what':<12}{'err_new':>12}{'err_torch':>12}{'bound':>12}  max|x|"]
    failures = []
    for i, name in enumerate(NAMES[:-1]):
        tst = topt.state[tparams[i]]
        for what, new, old, want, floor in (("param", params[i], tparams[i], truth.p[i], 1.0),
                                            ("exp_avg", mom[i][0], tst["exp_avg"], truth.m[i], 4.0),
                                            ("exp_avg_sq", mom[i][1], tst["exp_avg_sq"], truth.v[i], 4.0)):
            e_new, e_old, big = max_err(new, want), max_err(old, want), float(want.abs().max())
            bound = 2 * e_old + floor * ULP * big
            lines.append(f"  {name:<14}{what:<12}{e_new:>12.3e}{e_old:>12.3e}{bound:>12.3e}  {big:.3e}")
            if not e_new <= bound:
                failures.append(lines[-1])
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(REPO, "profiles", "fused_adamw_parity.txt"), "w") as fh:
        fh.write(text)
    assert not failures, "\n".join(failures)
    # the parameter whose .grad is None: bit-unchanged, and so are its (zero) moments
    assert torch.equal(params[-1].detach().cpu(), vals[-1])
    assert params[-1] not in opt.state or "exp_avg" not in opt.state[params[-1]]
    o = opt._offset[params[-1]]
    assert not opt.exp_avg[o:o + 100].any().item() and not opt.exp_avg_sq[o:o + 100].any().item()
    # the views moved their slice of the flat buffer and nothing around it
    untouched = torch.ones(FLAT, dtype=torch.bool)
    for o, n in VIEWS:
        untouched[o:o + n] = False
    assert torch.equal(params[len(SIZES)].flat_buffer.cpu()[untouched], flat[untouched])


def test_two_runs_are_bit_equal():
    """3: parameters, moments and the norm of two runs from the same state"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    steps = [make_grads(i, s) for i, s in enumerate(SCALES[:3])]
    a = run_fused(dev, vals, flat, steps)
    b = run_fused(dev, vals, flat, steps)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1].exp_avg, b[1].exp_avg) and torch.equal(a[1].exp_avg_sq, b[1].exp_avg_sq)
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    # another chunk size is another order of the f64 partial sums only: same update, norm within one rounding
    c = run_fused(dev, vals, flat, steps, chunk_elems=8192)
    for x, y in zip(a[2], c[2]):
        assert abs(float(x) - float(y)) <= ULP * float(x)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_skips_the_step(bad):
    """4: nothing moves, t stays, skipped goes up, the norm says why; the next finite step is step t + 1"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    params, opt, _ = run_fused(dev, vals, flat, [make_grads(0, 3e-4), make_grads(1, 3e-4)])
    assert opt.t == 2 and opt.skipped == 0
    before = [p.detach().clone() for p in params]
    m0, v0 = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    grads = make_grads(2, 3e-4)
    grads[5][17, 33] = bad
    keep = attach(params, grads, dev, [p.grad for p in params])
    norm = opt.step()
    assert not math.isfinite(float(norm))
    assert opt.t == 2 and opt.skipped == 1
    for p, q in zip(params, before):
        assert torch.equal(p, q)
    assert torch.equal(opt.exp_avg, m0) and torch.equal(opt.exp_avg_sq, v0)
    # the next finite step is the third one: equal to an uninterrupted run of three steps
    last = make_grads(3, 3e-4)
    attach(params, last, dev, keep)
    assert math.isfinite(float(opt.step()))
    assert opt.t == 3 and opt.skipped == 1
    want, wopt, _ = run_fused(dev, vals, flat, [make_grads(0, 3e-4), make_grads(1, 3e-4), last])
    for p, q in zip(params, want):
        assert torch.equal(p, q)
    assert torch.equal(opt.exp_avg, wopt.exp_avg) and torch.equal(opt.exp_avg_sq, wopt.exp_avg_sq)


def test_static_loss_scale_is_exact():
    """5: gradients times 2^14 with grad_scale = 2^-14: the bits of the unscaled run"""
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    steps = [make_grads(i, None, log_uniform=True) for i in range(3)]
    for g in steps[0][:-1]:
        assert 9.9e-7 <= float(g.abs().min()) and float(g.abs().max()) <= 1.01e2
    scaled = [[None if g is None else g * 2.0 ** 14 for g in grads] for grads in steps]
    a = run_fused(dev, vals, flat, steps)
    b = run_fused(dev, vals, flat, scaled, grad_scale=2.0 ** -14)
    assert float(a[1].result[1]) < 1.0                             # clipped: the coefficient is part of what must agree
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1].exp_avg, b[1].exp_avg) and torch.equal(a[1].exp_avg_sq, b[1].exp_avg_sq)
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def _model_and_optimizer(dev):
    import bench
    import optim
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    net = load_procedural(bench.build_model(0)).to(dev).train()
    zero_dropout(net)
    groups = [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
              {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": LRS[1]}]
    opt = optim.FusedAdamW(groups, lr=LRS[0], weight_decay=WD, max_norm=MAX_NORM)
    return net, opt


def test_in_the_captured_step():
    """6: (a) building the stepper leaves parameters and optimiser state alone; (b) three batches with a cosine schedule
    between them, through the in-graph optimiser and through an identical model whose optimiser steps after each replay:
    bit-equal parameters after every step, and the second step's update is the SCHEDULED learning rate's; (c) the first
    in-graph step against torch's AdamW + clip on the same gradients, under the parity bound; (d) it is a graph replay."""
    sys.path.insert(0, REPO)
    import bench
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(90 + i, 2, 8192, kind="room").to(dev) for i in range(3)]

    def criterion(ep, labels):
        return bench.loss_of(ep)

    net, opt = _model_and_optimizer(dev)
    names = [n for n, _ in net.named_parameters()]
    p0 = [p.detach().clone() for p in net.parameters()]
    st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, optimizer=opt)
    assert st.launch == "hipGraph replay"                                                    # (d)
    for n, p, q in zip(names, net.parameters(), p0):                                         # (a)
        assert torch.equal(p, q), n
    assert not opt.exp_avg.any().item() and not opt.exp_avg_sq.any().item()
    assert opt.t == 0 and opt.skipped == 0
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=3)

    net2, opt2 = _model_and_optimizer(dev)
    for p, q in zip(net2.parameters(), p0):
        assert torch.equal(p, q)
    st2 = train_step.CapturedStep(net2, criterion, {"point_clouds": pcs[0]})
    sched2 = torch.optim.lr_scheduler.CosineAnnealingLR(opt2, T_max=3)

    watch = "decoder.0.linear1.weight"
    wi = names.index(watch)
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        nx = None if nxt is None else {"point_clouds": nxt}
        before = [p.detach().clone() for p in net.parameters()]
        lr_now = opt.param_groups[1]["lr"]
        loss = st.step({"point_clouds": pc}, None, next_inputs=nx)
        assert torch.isfinite(loss).item() and math.isfinite(float(st.grad_total_norm))
        st2.step({"point_clouds": pc}, None, next_inputs=nx)
        opt2.step()
        torch.cuda.synchronize()
        assert opt.t == i + 1 and opt2.t == i + 1 and opt.skipped == 0
        builds = opt.table_builds
        for n, p, q in zip(names, net.parameters(), net2.parameters()):                     # (b)
            assert torch.equal(p, q), (i, n)
        assert any(not torch.equal(p, q) for p, q in zip(net.parameters(), before)), "the replay did not move the weights"
        if i == 0:                                                                           # (c)
            grads = [None if p.grad is None else p.grad.detach().clone() for p in net.parameters()]
            group = [1 if "decoder" in n else 0 for n in names]
            truth = Truth([q.cpu() for q in before])
            truth.step([None if g is None else g.cpu() for g in grads], group)
            tparams = [torch.nn.Parameter(q.clone()) for q in before]
            for p, g in zip(tparams, grads):
                p.grad = g
            topt = torch.optim.AdamW([{"params": [p for p, gi in zip(tparams, group) if gi == 0]},
                                      {"params": [p for p, gi in zip(tparams, group) if gi == 1], "lr": LRS[1]}],
                                     lr=LRS[0], weight_decay=WD, foreach=False)
            torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM, foreach=False)
            topt.step()
            worst, failures = (0.0, None), []
            for k, (n, p) in enumerate(zip(names, net.parameters())):
                if grads[k] is None:
                    assert torch.equal(p, before[k]), n
                    continue
                e_new, e_old = max_err(p, truth.p[k]), max_err(tparams[k], truth.p[k])
                bound = 2 * e_old + ULP * float(truth.p[k].abs().max())
                if bound > 0 and e_new / bound > worst[0]:
                    worst = (e_new / bound, n)
                if not e_new <= bound:
                    failures.append((n, e_new, e_old, bound))
            print(f"captured step vs torch: worst err_new / bound = {worst[0]:.3f} ({worst[1]}), "
                  f"{sum(g is not None for g in grads)} tensors with gradients")
            assert not failures, failures[:10]
        if i == 1:
            # the second step's update of one decoder weight, recomputed in f64 from the optimiser's own moments: it is the
            # SCHEDULED learning rate's (0.75 x the first step's after one cosine step of three), not the first step's
            assert abs(lr_now - 0.75 * LRS[1]) <= 1e-12
            p = list(net.parameters())[wi]
            m, v = (x.double() for x in (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))
            unit = m / (v.sqrt() / math.sqrt(1 - BETAS[1] ** 2) + EPS) / (1 - BETAS[0] ** 2)
            moved = before[wi].double() - p.detach().double()

            def miss(lr):
                return float((moved - (before[wi].double() * lr * WD + lr * unit)).abs().max()) / float(moved.abs().max())
            print(f"second step: miss with the scheduled lr {miss(lr_now):.3e}, with the first step's {miss(LRS[1]):.3e}")
            assert miss(lr_now) <= 1e-3 and miss(LRS[1]) >= 0.1
        sched.step()
        sched2.step()
    assert st.replays == 3 and builds == opt.table_builds            # the graph's gradient tensors are static: no rebuild


def test_checkpoint_continues_bit_identically(tmp_path):
    """7: save_checkpoint / load_checkpoint with FusedAdamW continues like an uninterrupted run, and a checkpoint written with
    torch.optim.AdamW loads into FusedAdamW"""
    import argparse
    import checkpoint
    dev = torch.device("cuda", 0)
    vals, flat = start_values()
    steps = [make_grads(i, 3e-4) for i in range(4)]

    class Holder(torch.nn.Module):
        def __init__(self, params):
            super().__init__()
            self.ps = torch.nn.ParameterList(params)

    want, wopt, _ = run_fused(dev, vals, flat, steps)
    params, opt, _ = run_fused(dev, vals, flat, steps[:2])
    model = Holder(params)
    sched = torch.optim.lr_scheduler.StepLR(opt, 100)
    args = argparse.Namespace(log_dir=str(tmp_path), save_freq=1, checkpoint_path=None)
    args.checkpoint_path = checkpoint.save_checkpoint(args, 1, model, opt, sched, save_cur=True)
    # a new process would start from fresh objects: other start values, zero moments, t = 0
    other, oflat = start_values(seed=5)
    params2 = device_params(other, oflat, dev)
    opt2 = fused_opt(params2)
    model2 = Holder(params2)
    assert checkpoint.load_checkpoint(args, model2, opt2, torch.optim.lr_scheduler.StepLR(opt2, 100)) == 1
    assert opt2.t == 2
    keep = None
    for grads in steps[2:]:
        keep = attach(params2, grads, dev, keep)
        opt2.step()
    torch.cuda.synchronize()
    assert opt2.t == 4
    for i, (p, q) in enumerate(zip(params2, want)):
        if i != len(NAMES) - 1:
            assert torch.equal(p, q), NAMES[i]
    for p, q in zip(params2[:-1], want[:-1]):
        assert torch.equal(opt2.state[p]["exp_avg"], wopt.state[q]["exp_avg"])
        assert torch.equal(opt2.state[p]["exp_avg_sq"], wopt.state[q]["exp_avg_sq"])
    # written with torch.optim.AdamW, read by FusedAdamW
    tparams = [torch.nn.Parameter(v.to(dev)) for v in vals]
    topt = torch.optim.AdamW(groups_of(tparams), lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD)
    for grads in steps[:2]:
        for p, g in zip(tparams, grads):
            p.grad = None if g is None else g.to(dev)
        topt.step()
    args.checkpoint_path = checkpoint.save_checkpoint(args, 2, Holder(tparams), topt, torch.optim.lr_scheduler.StepLR(topt, 100),
                                                      save_cur=True)
    params3 = device_params(other, oflat, dev)
    opt3 = fused_opt(params3)
    checkpoint.load_checkpoint(args, Holder(params3), opt3, torch.optim.lr_scheduler.StepLR(opt3, 100))
    assert opt3.t == 2
    for p, q in zip(params3[:-1], tparams[:-1]):
        assert torch.equal(p, q)
        assert torch.equal(opt3.state[p]["exp_avg"], topt.state[q]["exp_avg"])
        assert torch.equal(opt3.state[p]["exp_avg_sq"], topt.state[q]["exp_avg_sq"])
    assert params3[-1] not in opt3.state or not opt3.state[params3[-1]]
    attach(params3, steps[2], dev)
    assert math.isfinite(float(opt3.step())) and opt3.t == 3
