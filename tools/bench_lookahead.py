#!/usr/bin/env python
"""The captured training step with the sampling chain inside one step (CapturedStep(lookahead=1), what bench.py measures)
against the chain split over two steps (lookahead=2) at several cut points of the sa1 level.  The steppers are built the way
bench.py builds its own (bench.build_model, bench.loss_of, the same pool of clouds), all live in this one process and take
turns: every stepper is timed `--alternations` times over a window of at least `--seconds`, median ms per replay.

    python tools/bench_lookahead.py [--mean-teacher] [--head-rounds 1024,1433,1740] [--batch 8] [--points 40000]
"""
import argparse
import copy
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
import torch  # noqa: E402

import bench  # noqa: E402
import synth  # noqa: E402
import train_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--mean-teacher", action="store_true")
    ap.add_argument("--head-rounds", default="1024,1433,1740")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pool = [synth.make_clouds(100 + i, args.batch, args.points, kind="room").to(dev) for i in range(3)]
    tpool = [synth.make_clouds(200 + i, args.batch, args.points, kind="room").to(dev) for i in range(3)] \
        if args.mean_teacher else None
    torch.manual_seed(0)
    base = bench.build_model(0).to(dev).train()

    def criterion(ep, labels):
        return bench.loss_of(ep)

    configs = [("lookahead=1", 1, None)] + [(f"lookahead=2 head_rounds={int(k)}", 2, int(k))
                                            for k in args.head_rounds.split(",") if k]
    steppers = []
    for name, la, k in configs:
        net = copy.deepcopy(base)
        teacher = None
        if args.mean_teacher:
            teacher = copy.deepcopy(net)
            for p in teacher.parameters():
                p.detach_()
            teacher.train()
        st = train_step.CapturedStep(net, criterion, {"point_clouds": pool[0]}, teacher=teacher,
                                     teacher_example=None if teacher is None else {"point_clouds": tpool[0]},
                                     ema=bench.EMA_DECAY if teacher is not None else None, lookahead=la, head_rounds=k)
        assert st.launch == "hipGraph replay"
        steppers.append((name, st, la))
        print(f"built {name}: footprint {st.footprint or 'default (small inside forward)'}", flush=True)
    n = len(pool)

    def step(st, la, i):
        kw = {}
        if la == 2:
            kw["after_next_inputs"] = pool[(i + 2) % n]
            if tpool is not None:
                kw["after_next_teacher_inputs"] = tpool[(i + 2) % n]
        st.step(None, None, next_inputs=pool[(i + 1) % n], next_teacher_inputs=None if tpool is None else tpool[(i + 1) % n],
                **kw)
        if tpool is not None:
            st.update_teacher(bench.EMA_STEP + i)

    results = {name: [] for name, _, _ in steppers}
    counters = {name: 0 for name, _, _ in steppers}
    for alt in range(args.alternations):
        for name, st, la in steppers:
            i = counters[name]
            for _ in range(args.warmup):
                step(st, la, i)
                i += 1
            torch.cuda.synchronize()
            events = []
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.seconds or len(events) < 20:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(st, la, i)
                e1.record()
                events.append((e0, e1))
                i += 1
                if len(events) % 16 == 0:
                    torch.cuda.synchronize()          # keep the host at most a few replays ahead: the window is wall time
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3 / len(events)
            ms = statistics.median(a.elapsed_time(b) for a, b in events)
            counters[name] = i
            results[name].append(ms)
            print(f"run {alt} {name:34s} median {ms:7.3f} ms per replay ({len(events)} replays, {wall:7.3f} ms wall each)",
                  flush=True)
    import pointnet2_utils
    pointnet2_utils._ext.fps_check()
    kind = "mean-teacher step" if args.mean_teacher else "plain step"
    for name, _, _ in steppers:
        v = results[name]
        print(f"{kind}: {name:34s} median of runs {statistics.median(v):7.3f} ms (runs: {', '.join(f'{x:.3f}' for x in v)})")


if __name__ == "__main__":
    main()
