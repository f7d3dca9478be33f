#!/usr/bin/env python
"""What the ARKit physical-constraint loss (models/utils/arkit_loss_util.py, train.py:537) costs per call, forward +
backward, three ways, all live in one process and taking turns:

    (a) the device route, eager: omnipq_arkit_pc (2 launches) forward, omnipq_arkit_pc_grad (1 launch) backward
    (b) the same replayed from a hipGraph (what train_step.CapturedStep does with it)
    (c) the same mathematics as vectorised eager float32 torch ops on the GPU: every quad against every corner at once, no
        Python loop and no host read -- kinder than the reference, which loops over B x Q quads in Python

Every case is timed `--rounds` times (>= 5), interleaved, over a window of at least `--iters` calls and about 0.3 s that
ends in a device synchronise: WALL time per call, median and spread (max - min) over the rounds.  Inputs: the generator of
tests/arkit_inputs.py at Bu unlabelled scenes, Q quads and K2 boxes per scene, all boxes present.

`--step`: what the term costs INSIDE the mean-teacher step -- bench.py's `--mean-teacher` workload (PQ_Transformer, bf16,
batch 8, 40 000-point rooms, the step replayed from a hipGraph, the weight averaging after it), the batch read as 4 labelled
+ 4 unlabelled scenes, with semi_objective.SemiSupervisedObjective as the criterion (supervised loss, guide criterion,
consistency loss) and its ARKit term on or off; two child processes per variant, taking turns, ms per step over `--steps`
replays each.

Every measurement runs in a child process of its own under `--limit` seconds; a child that fails or runs out of time ends
the run.

    python tools/bench_arkit.py [--batch 8] [--quads 256] [--boxes 64] [--rounds 5] [--iters 20] [--limit 240]
    python tools/bench_arkit.py --step [--steps 40] [--limit 240]

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


def eager_loss(ep, unl):
    """include/omnipq_semi.h's mathematics in float32 torch ops; every label row must be a box (no padding)"""
    import torch
    cl, sl, counts = unl["center_label"], unl["size_label"], unl["num_gt_boxes"][..., 0]
    Bu = cl.shape[0]
    c, n = ep["last_quad_center"][Bu:, :, :2], ep["last_normal_vector"][Bu:, :, :2]
    gate = torch.softmax(ep["last_quad_scores"][Bu:], dim=-1)[..., 1] > 0.1
    rev = -(c.detach() * n.detach()).sum(-1) < 0
    ab = torch.where(rev[..., None], -n, n)
    sign = torch.tensor([[1.0, 1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, -1.0]], device=cl.device)
    P = (cl[:, :, None, :2] + sign * (sl[:, :, None, :2] / 2)).reshape(Bu, -1, 2)
    delta = torch.bmm(ab, P.transpose(1, 2)) - (ab * c).sum(-1, keepdim=True)
    t = P[:, None] - ab[:, :, None, :] * delta[..., None]
    inside = (t - c[:, :, None, :]).detach().norm(dim=-1) < ep["last_quad_size"][Bu:, :, 0:1].detach()
    pair = torch.relu(-delta) * inside
    loss = ((pair.sum(-1) / counts[:, None]) * gate).sum()
    collisions = ((pair.detach() > 1e-4) & gate[..., None]).sum()
    return loss, collisions


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def bench_term(Bu, Q, K2, rounds, iters):
    import torch
    import arkit_inputs
    from models.utils import arkit_loss_util as ak
    pred, unl = arkit_inputs.make((Bu, Q, K2, (K2,) * Bu), 500 + Bu, repair=False)
    ep = {k: torch.from_numpy(v).cuda() for k, v in pred.items()}
    batch = {k: torch.from_numpy(v).cuda() for k, v in unl.items()}
    leaves = [ep[k].requires_grad_(True) for k in ("last_quad_center", "last_normal_vector")]

    def device():
        loss, collisions = ak.get_arkit_pc_loss(ep, batch, None)
        return loss, collisions, torch.autograd.grad(loss, leaves)

    def eager():
        loss, collisions = eager_loss(ep, batch)
        return loss, collisions, torch.autograd.grad(loss, leaves)

    # Nothing attached to an autograd graph may be alive when the capture begins: a loss kept from a call on the default
    # stream keeps that call's AccumulateGrad nodes alive, and the captured backward then synchronises with the default
    # stream, which a capture does not survive.  So: warm-up on a side stream, capture, and only then the comparison.
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        device()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device()
    a, b = ([float(v.detach()) for v in fn()[:2]] for fn in (device, eager))
    agree = abs(a[0] - b[0]) / abs(b[0])
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
    out["loss"] = a[0]
    out["collisions"] = [a[1], b[1]]
    out["loss_rel_diff_device_vs_torch"] = agree
    return out


def bench_step(arkit, steps, warmup=10):
    """ms per replayed mean-teacher step (bench.py --mean-teacher's workload) with the objective, its ARKit term on or off"""
    import copy
    import types
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    import mt_inputs
    import semi_objective
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    B, half = 8, 4
    net = bench.build_model(0).to(dev).train()
    teacher = copy.deepcopy(net)
    for p in teacher.parameters():
        p.detach_()
    teacher.train()
    clouds = [synth.make_clouds(100 + i, B, 40000, kind="room") for i in range(3)]
    pool = [c.to(dev) for c in clouds]
    teacher_pool = [synth.make_clouds(200 + i, B, 40000, kind="room").to(dev) for i in range(3)]
    mean_size = bench.mean_size_arr()
    rng = np.random.default_rng(5)
    lab = synth.make_labels(clouds[0], 300, mean_size_arr=mean_size)
    size = mean_size[lab["size_class_label"].numpy()] + lab["size_residual_label"].numpy()
    normals = rng.standard_normal((half, 40000, 3))
    labels = {k: v[:half].to(dev) for k, v in lab.items()}
    labels.update({"unlabeled.center_label": lab["center_label"][half:].to(dev),
                   "unlabeled.size_label": torch.from_numpy(size[half:].astype(np.float32)).to(dev),
                   "unlabeled.num_gt_boxes": lab["num_gt_boxes"][half:].to(dev),
                   "unlabeled.point_clouds": pool[0][half:, :, :3].contiguous(),
                   "unlabeled.vertex_normals": torch.from_numpy(
                       (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(np.float32)).to(dev),
                   "consistency_weight": torch.tensor(1.0, device=dev)})
    for k, v in mt_inputs.augmentation(rng, B).items():
        labels[k], labels["unlabeled." + k] = torch.from_numpy(v[:half]).to(dev), torch.from_numpy(v[half:]).to(dev)

    class DatasetConfig(bench.LossConfig):
        mean_size_arr = mean_size

    cfg = types.SimpleNamespace(pc_loss=True, gamma_mixture=True, ema=True, arkit=bool(arkit), lambda_metric_normal=1.0,
                                lambda_metric_vertical=1.0, lambda_metric_size=1.0, lambda_metric_score=1.0,
                                lambda_arkit_pc_loss=1.0)
    objective = semi_objective.SemiSupervisedObjective(DatasetConfig, cfg)
    st = train_step.CapturedStep(net, objective, {"point_clouds": pool[0]}, labels, teacher=teacher,
                                 teacher_example={"point_clouds": teacher_pool[0]}, ema=bench.EMA_DECAY,
                                 teacher_to_criterion=True, warmup=3)
    assert st.launch == "hipGraph replay"

    def run(count, first):
        for i in range(first, first + count):
            st.step(None, labels, next_inputs=pool[(i + 1) % 3], next_teacher_inputs=teacher_pool[(i + 1) % 3])
            st.update_teacher(bench.EMA_STEP + i)

    run(warmup, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps, warmup)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return {"ms_per_step": ms, "arkit_pc_loss": float(objective.stats["arkit_pc_loss"]),
            "arkit_collisions": float(objective.stats["arkit_collisions"]), "total_loss": float(objective.stats["total_loss"])}


def child(cmd, limit, what):
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_arkit.py: {what} did not finish in {limit:.0f} s; stopping")
    if done.returncode != 0:
        sys.exit(f"bench_arkit.py: {what} failed ({done.returncode}); stopping\n{done.stderr[-2000:]}")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8, help="unlabelled scenes")
    ap.add_argument("--quads", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a child process may take")
    ap.add_argument("--step", action="store_true", help="the term inside the mean-teacher step instead")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-step", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    rounds = max(args.rounds, 5)
    if args.child:
        print(json.dumps(bench_term(args.batch, args.quads, args.boxes, rounds, args.iters)))
        return
    if args.child_step is not None:
        print(json.dumps(bench_step(bool(args.child_step), args.steps)))
        return
    me = [sys.executable, os.path.abspath(__file__)]
    if args.step:
        runs = {0: [], 1: []}
        for _ in range(2):
            for arkit in (0, 1):
                runs[arkit].append(child(me + ["--child-step", str(arkit), "--steps", str(args.steps)], args.limit,
                                         f"the step, arkit {arkit}"))
        times = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}
        base, term = statistics.mean(times[0]), statistics.mean(times[1])
        print(f"mean-teacher step (bench.py --mean-teacher's workload, 4 labelled + 4 unlabelled scenes, criterion "
              f"SemiSupervisedObjective), ms per replayed step over {args.steps} steps, two processes each, taking turns")
        print(f"  supervised + guide + consistency:            {times[0][0]:.3f} {times[0][1]:.3f}")
        print(f"  supervised + guide + consistency + ARKit:    {times[1][0]:.3f} {times[1][1]:.3f}")
        print(f"  the term costs {term - base:+.3f} ms per step ({100.0 * (term - base) / base:+.1f} %); its value in the last "
              f"step {runs[1][0]['arkit_pc_loss']:.4g}, {runs[1][0]['arkit_collisions']:.0f} collisions")
        print(json.dumps({"step_ms_without": times[0], "step_ms_with": times[1], "steps": args.steps, "runs": runs}))
        return
    r = child(me + ["--child", "--batch", str(args.batch), "--quads", str(args.quads), "--boxes", str(args.boxes), "--rounds",
                    str(rounds), "--iters", str(args.iters)], args.limit, "the term")
    print(f"ARKit physical-constraint loss, forward + backward, Bu = {args.batch}, Q = {args.quads}, K2 = {args.boxes} (all boxes "
          f"present); wall ms per call, median (spread) of {rounds} interleaved rounds; a round times each case over >= "
          f"{args.iters} calls and ~0.3 s")
    cell = lambda k: f"{r[k]['median_ms']:.3f} ({r[k]['spread_ms']:.3f})"      # noqa: E731
    print(f"  device, eager      {cell('device_eager')}")
    print(f"  device, hipGraph   {cell('device_graph')}")
    print(f"  torch ops, eager   {cell('torch_eager')}    {r['torch_eager']['median_ms'] / r['device_graph']['median_ms']:.1f}x the graph")
    print(f"  loss {r['loss']:.6g}, collisions {r['collisions'][0]:.0f} (torch ops: {r['collisions'][1]:.0f}), loss device vs "
          f"torch ops {r['loss_rel_diff_device_vs_torch']:.1e} relative")
    print(json.dumps(dict(r, batch=args.batch, quads=args.quads, boxes=args.boxes, rounds=rounds, iters=args.iters)))


if __name__ == "__main__":
    main()
