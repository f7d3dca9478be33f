#!/usr/bin/env python
"""A/B of the INFERENCE per-point stacks: rows_mlp.EVAL_CHAIN off (the stored route: per layer one GEMM, the launches that
rebuild the BatchNorm's constants and omnipq_bnrelu) against on (csrc/rows_infer.hip: the stack as one launch), on the benchmark
model in eval mode under torch.no_grad() and bf16 autocast.

    python tools/bench_rows_infer.py [--points 40000] [--batches 8 1] [--rounds 5] [--iters 200] [--out profiles/rows_infer_ab.txt]

Per batch size the five kinds of stack the eval forward runs are event-timed one by one through the model's own call sites, on
inputs of the model's shapes (1024 seeds and 256 proposals per scene): the position-embedding pair of two decoder layers
(decoder_rows.posembed_pair), the voting module, the object + quad head pair of a decoder stage (pred_heads.head_stack_pair)
and the two feature-propagation modules.  A call holds what the call site does besides the stack (the vote decode, the
three-neighbour interpolation) on both routes alike.  The whole eval forward is timed on the host clock, ending in a device
synchronise, in scenes/s -- as shipped (`forward`: the heads stay on the stored route, pred_heads._HEAD_EVAL_CHAIN) and with
the heads opted in as well (`forward+heads`); the head pair itself is measured with the switch on.  The two routes alternate
inside every round (same process, same inputs); the table reports the median over the rounds and the spread (max - min) next to
it.  A kind's verdict is `chain` when the chain's median is below the stored route's by more than the two spreads together, at
EVERY batch size.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402

NAMES = ["pos_pair", "vote", "head_pair", "fp1", "fp2"]


def stack_calls(net, B, dev):
    """-> {kind: (callable, chain launches per call)} on inputs of the model's shapes"""
    import decoder_rows
    import pred_heads
    gen = torch.Generator(device=dev).manual_seed(5)

    def rand(*shape, scale=1.0):
        return torch.randn(shape, device=dev, generator=gen) * scale

    bb = net.backbone
    c3, c2 = bb.fp1.mlp[0].conv.in_channels // 2, bb.fp2.mlp[0].conv.in_channels - bb.fp1.mlp[-1].conv.out_channels
    key_xyz = rand(B, 1024, 3, scale=2.0)
    seed_xyz, seed_feat = rand(B, 1024, 3, scale=2.0), rand(B, 288, 1024)
    feat, feat_q = rand(B, 288, 256), rand(B, 288, 256)
    xyz2, xyz3, xyz4 = rand(B, 1024, 3, scale=2.0), rand(B, 512, 3, scale=2.0), rand(B, 256, 3, scale=2.0)
    f3, f4 = rand(B, c3, 512), rand(B, c3, 256)
    f2, f1out = rand(B, c2, 1024), rand(B, bb.fp1.mlp[-1].conv.out_channels, 512)
    pe = net.decoder_cross_posembeds
    return {
        "pos_pair": (lambda: decoder_rows.posembed_pair(pe[0], pe[1], key_xyz), 2),
        "vote": (lambda: net.vote(seed_xyz, seed_feat, normalized=True), 1),
        "head_pair": (lambda: pred_heads.head_stack_pair(net.prediction_heads[0], net.prediction_quad_heads[0], feat, feat_q), 2),
        "fp1": (lambda: bb.fp1(xyz3, xyz4, f3, f4), 1),
        "fp2": (lambda: bb.fp2(xyz2, xyz3, f2, f1out), 1),
    }


def first_tensor(out):
    while not torch.is_tensor(out):
        out = out[0]
    return out


def time_call(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_forward(net, pc, iters):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            net({"point_clouds": pc})
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rows_infer_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rows_infer: needs a GPU (nothing is timed without one)")
    import pred_heads
    import rows_mlp
    import synth
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = bench.build_model(0).to(dev).eval()
    shipped, shipped_heads = rows_mlp.EVAL_CHAIN, pred_heads._HEAD_EVAL_CHAIN
    pred_heads._HEAD_EVAL_CHAIN = True           # the head pair is measured on the chain like the others (shipped off)
    lines = [f"# python tools/bench_rows_infer.py --points {args.points} --batches {' '.join(map(str, args.batches))} "
             f"--rounds {args.rounds} --iters {args.iters}        ({torch.cuda.get_device_name(0)}, one process)",
             "# eval / no_grad / bf16; stored = rows_mlp.EVAL_CHAIN off, chain = on, alternating inside every round; ms per call: "
             "median over the rounds (spread = max - min)"]
    wins = {n: True for n in NAMES}
    for B in args.batches:
        pc = synth.make_clouds(100, B, args.points, kind="room").to(dev)
        calls = stack_calls(net, B, dev)
        # the route under test is the one that runs, and the two compute the same function on the inputs that are timed
        outs, forward_chains = {}, {}
        for mode in (False, True):
            rows_mlp.EVAL_CHAIN = mode
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                outs[mode] = {}
                for n, (fn, launches) in calls.items():
                    uses = rows_mlp.eval_chain_uses
                    outs[mode][n] = first_tensor(fn()).float()
                    ran = rows_mlp.eval_chain_uses - uses
                    assert ran == (launches if mode else 0), f"{n}: {ran} chain launches with EVAL_CHAIN = {mode}"
                for heads in (False, True, False, True):     # warm-up of the whole forward, every configuration timed
                    pred_heads._HEAD_EVAL_CHAIN = heads
                    uses = rows_mlp.eval_chain_uses
                    net({"point_clouds": pc})
                    forward_chains[mode, heads] = rows_mlp.eval_chain_uses - uses
        assert forward_chains[False, False] == forward_chains[False, True] == 0
        lines.append(f"# batch {B}: the whole eval forward runs {forward_chains[True, False]} stacks on the chain as shipped (the "
                     f"heads on the stored route), {forward_chains[True, True]} with the heads opted in (forward+heads)")
        for n in NAMES:
            a, b = outs[False][n], outs[True][n]
            rel = float((a - b).norm() / a.norm())
            lines.append(f"# batch {B} {n}: chain against stored, rel-L2 of the call's first output {rel:.2e}")
            assert rel < 0.125, (n, rel)                     # 32 u of bf16: see tests/test_gpu_rows_infer.py
        t = {(n, m): [] for n in NAMES + ["forward", "forward+heads"] for m in (False, True)}
        for _ in range(args.rounds):
            for mode in (False, True):
                rows_mlp.EVAL_CHAIN = mode
                for n in NAMES:
                    time_call(calls[n][0], 2)
                    t[n, mode].append(time_call(calls[n][0], args.iters))
                # the whole forward as shipped (the heads on the stored route), and with the heads opted in as well
                for n, heads in (("forward", False), ("forward+heads", True)):
                    pred_heads._HEAD_EVAL_CHAIN = heads
                    time_forward(net, pc, 2)
                    t[n, mode].append(time_forward(net, pc, max(args.iters // 2, 3)))      # about a second per sample
                pred_heads._HEAD_EVAL_CHAIN = True
        for n in NAMES + ["forward", "forward+heads"]:
            med = {m: statistics.median(t[n, m]) for m in (False, True)}
            spr = {m: max(t[n, m]) - min(t[n, m]) for m in (False, True)}
            faster = med[True] < med[False] - (spr[False] + spr[True])
            if n in wins:
                wins[n] &= faster
            extra = ""
            if n.startswith("forward"):
                extra = f"   {B / med[False] * 1e3:8.1f} -> {B / med[True] * 1e3:8.1f} scenes/s"
            lines.append(f"batch {B} {n:13s} stored {med[False]:8.4f} ms ({spr[False]:.4f})   chain {med[True]:8.4f} ms "
                         f"({spr[True]:.4f})   stored / chain {med[False] / med[True]:5.2f}   "
                         f"{'chain faster' if faster else 'not faster beyond the spreads'}{extra}")
    rows_mlp.EVAL_CHAIN, pred_heads._HEAD_EVAL_CHAIN = shipped, shipped_heads
    for n in NAMES:
        lines.append(f"verdict {n}: {'chain' if wins[n] else 'stored'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
