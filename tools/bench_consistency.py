#!/usr/bin/env python
"""What the mean-teacher consistency loss (models/utils/mean_teacher_consistency_util.py, train.py:531) costs per call,
forward + backward over all seven prediction heads and both kinds, three ways, all live in one process and taking turns:

    (a) the device route, eager: omnipq_mt_consistency (3 launches) forward, omnipq_mt_consistency_grad (1 launch) backward
    (b) the same replayed from a hipGraph (what train_step.CapturedStep does with it)
    (c) the same mathematics as eager float32 torch ops on the GPU, written the way the reference writes it: a Python loop
        over the prefixes, `nonzero` for the flips, K x K distance tensors, per-scene list comprehensions for the gathers,
        `torch.quantile` -- fourteen times about sixty small ops

Every case is timed `--rounds` times (>= 5), interleaved, over a window of at least `--iters` calls and about 0.3 s that
ends in a device synchronise: WALL time per call, median and spread (max - min) over the rounds.  Inputs: the structured
case of tests/mt_inputs.py (the teacher a noisy permutation of the student) at K proposals.

Every batch size runs in a child process of its own under `--limit` seconds; a child that fails or runs out of time ends
the run.

`--step`: what the term costs INSIDE the mean-teacher step -- bench.py's `--mean-teacher` workload (PQ_Transformer, bf16,
batch 8 + 8, 40 000-point rooms, the step replayed from a hipGraph, the weight averaging after it) with the criterion
`loss_of(end_points)` and with `loss_of(end_points) + get_consistency_loss(...)`, `teacher_to_criterion=True` in both; two
child processes per variant, taking turns, ms per step over `--steps` replays each.

    python tools/bench_consistency.py [--batches 8,16] [--proposals 256] [--rounds 5] [--iters 20] [--limit 240]
    python tools/bench_consistency.py --step [--steps 40] [--limit 240]

Prints a table and one JSON line (last line of the output).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))


def take(x, a):
    import torch
    return torch.cat([torch.index_select(xb, 0, ab).unsqueeze(0) for xb, ab in zip(x, a)])


def clip(v):
    import torch
    eps = torch.quantile(v, 0.85)
    return torch.mean((v < eps) * v)


def eager_centre(S, T, p, centre, score):
    import torch
    import torch.nn.functional as F
    e = T[p + centre].clone()                                   # the reference flips the teacher's tensor itself
    fx = torch.nonzero(S["flip_x_axis"]).squeeze(1)             # host read
    e[fx, :, 0] = -e[fx, :, 0]
    fy = torch.nonzero(S["flip_y_axis"]).squeeze(1)             # host read
    e[fy, :, 1] = -e[fy, :, 1]
    e = torch.bmm(e, S["rot_mat"].transpose(1, 2))
    e = e * S["scale"].reshape(-1, 1, 1)
    c = S[p + centre]
    K = c.shape[1]
    dist = torch.sum((c.unsqueeze(2).repeat(1, 1, K, 1) - e.unsqueeze(1).repeat(1, K, 1, 1)) ** 2, dim=-1)
    dist1, ind1 = torch.min(dist, dim=2)
    dist2, ind2 = torch.min(dist, dim=1)
    s = F.softmax(S[p + score], dim=2)[..., 1]
    d = dist1 * torch.stack([sc[i] for sc, i in zip(s, ind1)], dim=0) + dist2 * s
    return clip(d), ind2, s


def eager_loss(S, T, mean_size, prefixes):
    import torch
    import torch.nn.functional as F
    total = torch.zeros((), device=mean_size.device)
    scale = S["scale"].reshape(-1, 1, 1)
    for p in prefixes:
        centre, a, s = eager_centre(S, T, p, "center", "objectness_scores")
        log_p = take(F.log_softmax(S[p + "sem_cls_scores"], dim=2), a)
        cls = 2 * F.kl_div(log_p, F.softmax(T[p + "sem_cls_scores"], dim=2), reduction="mean")
        sizes = []
        for ep in (S, T):
            c = torch.argmax(ep[p + "size_scores"], -1)
            res = torch.gather(ep[p + "size_residuals"], 2, c.unsqueeze(-1).unsqueeze(-1).expand(-1, -1, -1, 3)).squeeze(2)
            sizes.append(torch.index_select(mean_size, 0, c.view(-1)).view(res.shape) + res)
        size = clip(torch.sum((take(sizes[0], a) - sizes[1] * scale) ** 2, dim=2) * s)
        total = total + 0.5 * centre + cls + 0.05 * size
        centre, a, s = eager_centre(S, T, p, "quad_center", "quad_scores")
        cos = F.cosine_similarity(take(S[p + "normal_vector"], a)[..., :2], T[p + "normal_vector"][..., :2], dim=2)
        normal = clip((1.0 - cos.abs()) * s)
        size = clip(torch.sum((take(S[p + "quad_size"], a) - T[p + "quad_size"]) ** 2, dim=2) * s)
        log_p = take(F.log_softmax(S[p + "quad_scores"], dim=2), a)
        cls = 2 * F.kl_div(log_p, F.softmax(T[p + "quad_scores"], dim=2), reduction="batchmean")
        total = total + 0.5 * centre + 0.0 * cls + normal + 0.05 * size
    return total / len(prefixes)


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def bench_batch(B, K, rounds, iters):
    import warnings
    import torch
    import mt_inputs
    from models.utils import mean_teacher_consistency_util as mt
    warnings.filterwarnings("ignore", message="reduction")
    S_np, T_np, mean_size = mt_inputs.make((B, K, 18, 18), 500 + B, structured=True)
    S = {k: torch.from_numpy(v).cuda() for k, v in S_np.items()}
    T = {k: torch.from_numpy(v).cuda() for k, v in T_np.items()}
    names = [p + k for p in mt_inputs.PREFIXES for k in mt_inputs.GRAD_KEYS]
    leaves = [S[k].requires_grad_(True) for k in names]
    cfg = mt_inputs.Config(18)
    ms = torch.from_numpy(mean_size).cuda()

    def device():
        loss, _ = mt.get_consistency_loss(dict(S), T, cfg)
        return loss, torch.autograd.grad(loss, leaves)

    def eager():
        loss = eager_loss(S, T, ms, mt_inputs.PREFIXES)
        return loss, torch.autograd.grad(loss, leaves)

    agree = abs(float(device()[0]) - float(eager()[0])) / abs(float(eager()[0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        device()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device()
    cases = {"device_eager": device, "device_graph": graph.replay, "torch_eager": eager}
    for fn in cases.values():
        fn()                                                    # warm-up
    # a window of at least `iters` calls and at least ~0.3 s: a 0.1 ms call timed over 2 ms measures the scheduler
    window = {k: max(iters, int(300.0 / max(timed(fn, 5), 1e-3)) + 1) for k, fn in cases.items()}
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():                             # interleaved: every round times every case once
            times[k].append(timed(fn, window[k]))
    out = {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "calls_per_window": window[k]}
           for k, v in times.items()}
    out["loss_rel_diff_device_vs_torch"] = agree
    return out


def bench_step(with_term, steps, warmup=10):
    """ms per replayed mean-teacher step (bench.py --mean-teacher's workload) with or without the term in the criterion"""
    import copy
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    import mt_inputs
    import synth
    import train_step
    from models.utils import mean_teacher_consistency_util as mt
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    net = bench.build_model(0).to(dev).train()
    teacher = copy.deepcopy(net)
    for p in teacher.parameters():
        p.detach_()
    teacher.train()
    pool = [synth.make_clouds(100 + i, 8, 40000, kind="room").to(dev) for i in range(3)]
    teacher_pool = [synth.make_clouds(200 + i, 8, 40000, kind="room").to(dev) for i in range(3)]
    aug = {k: torch.from_numpy(v).to(dev) for k, v in mt_inputs.augmentation(np.random.default_rng(5), 8).items()}
    cfg = mt_inputs.Config(18)
    cfg.mean_size_arr = bench.mean_size_arr()

    def criterion(ep, labels, teacher_ep):
        loss = bench.loss_of(ep)
        if with_term:
            ep.update(aug)
            loss = loss + mt.get_consistency_loss(ep, teacher_ep, cfg)[0]
        return loss

    st = train_step.CapturedStep(net, criterion, {"point_clouds": pool[0]}, None, teacher=teacher,
                                 teacher_example={"point_clouds": teacher_pool[0]}, ema=bench.EMA_DECAY,
                                 teacher_to_criterion=True, warmup=3)
    assert st.launch == "hipGraph replay"

    def run(count, first):
        for i in range(first, first + count):
            st.step(None, None, next_inputs=pool[(i + 1) % 3], next_teacher_inputs=teacher_pool[(i + 1) % 3])
            st.update_teacher(bench.EMA_STEP + i)

    run(warmup, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps, warmup)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def child(cmd, limit, what):
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_consistency.py: {what} did not finish in {limit:.0f} s; stopping")
    if done.returncode != 0:
        sys.exit(f"bench_consistency.py: {what} failed ({done.returncode}); stopping\n{done.stderr[-2000:]}")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,16")
    ap.add_argument("--proposals", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a batch size may take")
    ap.add_argument("--step", action="store_true", help="the term inside the mean-teacher step instead")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-step", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    if args.child is not None:
        print(json.dumps(bench_batch(args.child, args.proposals, rounds, args.iters)))
        return
    if args.child_step is not None:
        print(json.dumps({"ms_per_step": bench_step(bool(args.child_step), args.steps)}))
        return
    if args.step:
        times = {0: [], 1: []}
        for _ in range(2):
            for with_term in (0, 1):
                cmd = [sys.executable, os.path.abspath(__file__), "--child-step", str(with_term), "--steps", str(args.steps)]
                times[with_term].append(child(cmd, args.limit, f"the step, term {with_term}")["ms_per_step"])
        base, term = statistics.mean(times[0]), statistics.mean(times[1])
        print(f"mean-teacher step (bench.py --mean-teacher's workload, teacher_to_criterion=True), ms per replayed step over "
              f"{args.steps} steps, two processes each, taking turns")
        print(f"  criterion loss_of(ep):                          {times[0][0]:.3f} {times[0][1]:.3f}")
        print(f"  criterion loss_of(ep) + get_consistency_loss:   {times[1][0]:.3f} {times[1][1]:.3f}")
        print(f"  the term costs {term - base:+.3f} ms per step ({100.0 * (term - base) / base:+.1f} %)")
        print(json.dumps({"step_ms_without": times[0], "step_ms_with": times[1], "steps": args.steps}))
        return
    out = {"proposals": args.proposals, "rounds": rounds, "iters": args.iters, "batches": {}}
    print(f"mean-teacher consistency loss, forward + backward, 7 prefixes x 2 kinds, K = {args.proposals}; wall ms per call, "
          f"median (spread) of {rounds} interleaved rounds; a round times each case over >= {args.iters} calls and ~0.3 s")
    print(f"{'B':>3} {'device, eager':>22} {'device, hipGraph':>22} {'torch ops, eager':>22} {'torch / graph':>14}")
    for B in (int(b) for b in args.batches.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--proposals", str(args.proposals), "--rounds",
               str(rounds), "--iters", str(args.iters)]
        r = child(cmd, args.limit, f"B = {B}")
        out["batches"][str(B)] = r
        cell = lambda k: f"{r[k]['median_ms']:.3f} ({r[k]['spread_ms']:.3f})"      # noqa: E731
        print(f"{B:>3} {cell('device_eager'):>22} {cell('device_graph'):>22} {cell('torch_eager'):>22} "
              f"{r['torch_eager']['median_ms'] / r['device_graph']['median_ms']:>13.1f}x", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
