#!/usr/bin/env python
"""What the gamma-mixture guide criterion (models/utils/gamma_mixture_loss_util.py, train.py:513) costs per call, forward +
backward, three ways, all live in one process and taking turns:

    (a) the device route, eager: omnipq_gm_draw + omnipq_gm_guide (2 launches) forward, omnipq_gm_guide_grad backward
    (b) the same replayed from a hipGraph (what train_step.CapturedStep does with it)
    (c) the same math as eager torch ops on the GPU, written the way the reference writes it: a Python loop over the scenes,
        `random.choice` over the candidate quads, `torch.randint` on the host, about sixty small ops per scene and the host
        reads the reference has (`kept.shape[0] < 300`, `.item()`, the three `if`s on device scalars).  The keep mask is
        `|t| <= T_STAR` on the device: the host fit (fit.py `fit_gamma`: 25 EM steps with scipy.optimize.root, then a Python
        loop over the 10 000 samples) is NOT in (c).

Every case is timed `--rounds` times (>= 5), interleaved, over a window of at least `--iters` calls and about 0.3 s that
ends in a device synchronise: WALL time per call, median and spread (max - min) over the rounds.  Scenes: the box room of
tests/gm_inputs.py with the wall quad of its case "a" (every scene is computed, none skipped).

`--host-fit DIR` (no GPU needed): time `fit_gamma` of DIR/fit.py -- the reference's, imported in place -- on the distances
of one scene, per scene; reported separately because it is host work that (c) leaves out.

    python tools/bench_gamma_mixture.py [--batches 4,8] [--points 40000] [--samples 10000] [--rounds 5] [--iters 20]

Prints a table and one JSON line (last line of the output).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gm_inputs  # noqa: E402

T_STAR = 0.29961316955346434
LEAVES = ("last_quad_scores", "last_quad_center", "last_quad_size")


def sl1(e):
    d = e.abs()
    return torch.where(d < 1.0, 0.5 * d * d, d - 0.5)


def eager_scene(xyz, normals, score, center, nv, size, K):
    """One scene of (c): float32 torch ops on the device, with the reference's host reads."""
    dev = xyz.device
    inds = torch.randint(0, xyz.shape[0], (K,))
    x, m = xyz[inds, :3], normals[inds]
    s0 = size[0] / 1.5
    n = torch.cat([nv[:2] / nv[:2].norm().detach(), torch.zeros(1, device=dev)]).detach()
    xdir = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], device=dev), n)
    mh = m / m.norm(dim=1)[:, None].clamp(min=1e-5)
    dc = 1.0 - (mh @ n).abs()
    o = x - center
    v = (o @ n).abs()
    xz = torch.stack([(o @ xdir).abs(), o[:, 2].abs()], dim=1)
    a = (2 * xz - torch.stack([s0, size[1]])).clamp(min=0.0).norm(dim=-1)
    total = 2.5 * dc + 0.2 * a ** 2 + 0.5 * v
    keep = total.detach().abs() <= T_STAR                       # stands in for the host fit
    kept, kept_m = x[keep], m[keep]
    zero = torch.zeros((), device=dev)
    if kept.shape[0] < 300:                                     # host read
        return zero, zero, zero, zero
    est = torch.cat([kept_m.mean(0)[:2], torch.zeros(1, device=dev)])
    est = est / est.norm()
    mn = 1.0 - torch.cosine_similarity(est[None], n[None]).abs().item()        # host read
    vk = v[keep]
    mv = (vk * (vk < torch.quantile(vk, 0.85))).mean()
    mu = kept.mean(0)
    xdp = ((x - mu) @ xdir).abs()[keep]
    px = torch.stack([torch.quantile(xdp, t) / t for t in (0.85, 0.925, 1.0)]).mean()
    ms = sl1(s0 - 2 * torch.tensor([px.item()], device=dev)).sum() + sl1(mu - center).sum()      # host read
    ce = torch.nn.CrossEntropyLoss()
    if mv < 0.05 and mn < 0.02 and ms < 0.10:                   # host reads
        msc = ce(score[None], torch.ones(1, dtype=torch.long, device=dev))
    elif mv > 0.3 or mn > 0.05 or ms > 0.35:
        msc = ce(score[None], torch.zeros(1, dtype=torch.long, device=dev))
    else:
        msc = zero
    return torch.tensor(mn, device=dev), mv, ms, msc


def eager_criterion(ep, K):
    sums = [torch.zeros((), device=ep["point_clouds"].device) for _ in range(4)]
    masks = torch.softmax(ep["last_quad_scores"], dim=-1)[..., 1] > 0.1
    B = masks.shape[0]
    for b in range(B):
        cand = torch.where(masks[b])[0]
        if cand.shape[0] == 0:                                  # host read
            continue
        j = random.choice(cand)
        terms = eager_scene(ep["point_clouds"][b], ep["vertex_normals"][b], ep["last_quad_scores"][b, j],
                            ep["last_quad_center"][b, j], ep["last_normal_vector"][b, j], ep["last_quad_size"][b, j], K)
        sums = [s + t for s, t in zip(sums, terms)]
    return [s / B for s in sums]


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def bench_batch(B, N, K, rounds, iters):
    from models.utils import gamma_mixture_loss_util as gm
    scenes = [gm_inputs.make(500 + b, "a", n=N) for b in range(B)]
    ep = {k: torch.from_numpy(v).cuda() for k, v in gm_inputs.batch(scenes).items()}
    leaves = [ep[k].requires_grad_(True) for k in LEAVES]

    def device():
        terms = gm.gamma_mixture_guide_criterion(ep, None, None, K=K)
        return torch.autograd.grad(terms[1] + terms[2] + terms[3], leaves)

    def eager():
        terms = eager_criterion(ep, K)
        return torch.autograd.grad(terms[1] + terms[2] + terms[3], leaves, allow_unused=True)

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
    return {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "calls_per_window": window[k]}
            for k, v in times.items()}


def host_fit(ref_dir, K):
    """seconds per scene of the reference's fit_gamma on the distances of one scene of case "a" (CPU)"""
    import types
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, ref_dir)
    stub = types.ModuleType("IPython")
    stub.embed = None
    sys.modules.setdefault("IPython", stub)
    import fit
    import gm_restatement as R
    sc = gm_inputs.make(500, "a")
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(a).double()                  # noqa: E731
    j = gm_inputs.SLOTS[0]
    d = R.distances(t(sc["point_clouds"]), t(sc["vertex_normals"]), t(sc["last_quad_center"][j]),
                    t(sc["last_normal_vector"][j]), t(sc["last_quad_size"][j]), torch.from_numpy(rng.integers(0, gm_inputs.N, K)))
    arr = d["total"].numpy().astype(np.float32)
    old = np.seterr(all="ignore")
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        fit.fit_gamma(arr, a1=2, b1=20, a2=3, b2=1, weight=0.1, step=25, save=None, quiet=True)
        times.append(time.perf_counter() - t0)
    np.seterr(**old)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,8")
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-fit", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.host_fit:
        s = host_fit(args.host_fit, args.samples)
        print(f"fit_gamma on {args.samples} distances (CPU, median of 3): {s:.3f} s per scene")
        print(json.dumps({"host_fit_s_per_scene": s, "samples": args.samples}))
        return
    rounds = max(args.rounds, 5)
    out = {"points": args.points, "samples": args.samples, "rounds": rounds, "iters": args.iters,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    print(f"gamma-mixture guide, forward + backward, N = {args.points}, K = {args.samples}; wall ms per call, "
          f"median (spread) of {rounds} interleaved rounds; a round times each case over >= {args.iters} calls and ~0.3 s")
    print(f"{'B':>3} {'device, eager':>22} {'device, hipGraph':>22} {'torch ops + host reads':>26} {'eager / graph':>14}")
    for B in (int(b) for b in args.batches.split(",")):
        r = bench_batch(B, args.points, args.samples, rounds, args.iters)
        out["batches"][str(B)] = r
        cell = lambda k: f"{r[k]['median_ms']:.3f} ({r[k]['spread_ms']:.3f})"      # noqa: E731
        print(f"{B:>3} {cell('device_eager'):>22} {cell('device_graph'):>22} {cell('torch_eager'):>26} "
              f"{r['torch_eager']['median_ms'] / r['device_graph']['median_ms']:>13.1f}x")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
