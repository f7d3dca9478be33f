#!/usr/bin/env python
"""What the three weight-changing lines of the training step (train.py:562-566) cost on the procedural PQ_Transformer with the
reference's two parameter groups (train.py:364-374), eleven ways, all live in one process and taking turns:

    (a) torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW as train.py constructs it        what a user ran before optim.py
    (b) the same with fused=True
    (c) optim.FusedAdamW.step(), eager                                                       three HIP launches
    (d) a replayed train_step.CapturedStep with the FusedAdamW inside the graph
    (e) a replayed CapturedStep without optimiser, followed by (a)
    (f) gradient accumulation over two micro-batches inside the graph: a replayed CapturedStep(step_freq=2) with
        FusedAdamW(accum_steps=2); one iteration = one micro-batch
    (g) the same accumulation from the host: a replayed CapturedStep without optimiser, the 519 gradient tensors copied
        (first micro-batch) or added (second, torch._foreach_add_) into tensors of the caller's, FusedAdamW.step() on the
        sum every second call; one iteration = one micro-batch
    (h) optim.FusedAdamW.step() with an attached teacher (attach_teacher): the mean-teacher weight averaging of
        train.py:435-439 inside the same three launches -- 36 bytes per parameter
    (i) optim.FusedAdamW.step() followed by ema.update_ema_variables: the averaging as a fourth launch -- 40 bytes per parameter
    (j) the mean-teacher step (student forward + backward, teacher forward, clip + AdamW, averaging) as ONE replay:
        CapturedStep(teacher=..., optimizer=FusedAdamW, ema_in_step=True)
    (k) the same step as a replay followed by stepper.update_teacher(global_step)

Every case is timed `--rounds` times (>= 5), interleaved, over a window of `--iters` iterations that ends in a device
synchronise: WALL time per iteration, median and spread (max - min) over the rounds.  A last pass runs a few iterations of
every case under torch.profiler and sums the device time of its kernels.  For (c) the traffic the arithmetic needs (32 bytes
per parameter: the norm reads g, the update reads p, g, m, v and writes p, m, v) over the time is set against 8 TB/s and
against the 6.25 TB/s the project's copy probe reaches.  `--chunks` times (c) at other chunk sizes as well.  The accumulate
launch of (f) (omnipq_adamw_accum_sqnorm: reads the gradient and the sum, writes the sum -- 12 bytes per parameter) is timed
on its own: an eager FusedAdamW(accum_steps=10**6) never reaches its applying call, so every step() after the first is that
launch on a non-first micro-batch plus a finalise and an update that return at once.

Learning rates are tiny on purpose (time does not depend on them): hundreds of steps on the stand-in loss must not drive
the weights to a non-finite gradient norm, which FusedAdamW would answer by skipping the update -- `skipped` is checked.

    python tools/bench_optimizer.py [--batch 8] [--points 40000] [--rounds 5] [--iters 40] [--chunks 4096,8192,16384]

Prints one JSON line (last line of the output).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import torch  # noqa: E402

import bench  # noqa: E402
import optim  # noqa: E402
import synth  # noqa: E402
import train_step  # noqa: E402

LR, DECODER_LR, WD, CLIP = 1e-6, 1e-7, 5e-4, 0.1


def groups(net):
    return [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
            {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": DECODER_LR}]


def kernel_time_ms(fn, iters, match=None):
    """summed device time of everything `fn` launches (match: of the kernels whose name contains it), per call
    (torch.profiler, a pass of its own); None: not measured"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        total = 0.0
        for e in prof.key_averages():
            total += getattr(e, "self_device_time_total", None) or getattr(e, "self_cuda_time_total", 0.0) or 0.0
        if match is not None:
            total = 0.0
            for e in prof.key_averages():
                if match in e.key:
                    total += getattr(e, "self_device_time_total", None) or getattr(e, "self_cuda_time_total", 0.0) or 0.0
        return total / 1e3 / iters if total > 0 else None
    except Exception as exc:  # the figure is reported as not measured, never guessed
        print(f"kernel time not measured: {type(exc).__name__}: {exc}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunks", default="", help="further FusedAdamW chunk sizes to time as (c), comma separated")
    ap.add_argument("--no-kernel-time", action="store_true")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: at least 5 interleaved rounds")
    dev = torch.device("cuda", 0)
    from procedural import load_procedural
    base = load_procedural(bench.build_model(0)).to(dev).train()
    nparam = sum(p.numel() for p in base.parameters())
    ntensor = sum(1 for _ in base.parameters())
    pool = [synth.make_clouds(100 + i, args.batch, args.points, kind="room").to(dev) for i in range(3)]

    def criterion(ep, labels):
        return bench.loss_of(ep)

    def with_static_grads(net):
        g = torch.Generator(device=dev).manual_seed(1)
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-5       # norm ~ 0.04: under the clip, so (a) / (b)
        return net                                                              # do not shrink it step after step

    cases = {}
    net_a = with_static_grads(copy.deepcopy(base))
    opt_a = torch.optim.AdamW(groups(net_a), lr=LR, weight_decay=WD)
    pa = list(net_a.parameters())

    def run_a():
        torch.nn.utils.clip_grad_norm_(pa, CLIP)
        opt_a.step()
    cases["a_torch_adamw_clip"] = run_a

    net_b = with_static_grads(copy.deepcopy(base))
    opt_b = torch.optim.AdamW(groups(net_b), lr=LR, weight_decay=WD, fused=True)
    pb = list(net_b.parameters())

    def run_b():
        torch.nn.utils.clip_grad_norm_(pb, CLIP)
        opt_b.step()
    cases["b_torch_adamw_fused_clip"] = run_b

    fused = {}
    for chunk in [optim.CHUNK] + [int(c) for c in args.chunks.split(",") if c and int(c) != optim.CHUNK]:
        net_c = with_static_grads(copy.deepcopy(base))
        opt_c = optim.FusedAdamW(groups(net_c), lr=LR, weight_decay=WD, max_norm=CLIP, chunk_elems=chunk)
        name = "c_fused_adamw_eager" + ("" if chunk == optim.CHUNK else f"_chunk{chunk}")
        fused[name] = opt_c
        cases[name] = opt_c.step

    net_d = copy.deepcopy(base)
    opt_d = optim.FusedAdamW(groups(net_d), lr=LR, weight_decay=WD, max_norm=CLIP)
    st_d = train_step.CapturedStep(net_d, criterion, {"point_clouds": pool[0]}, optimizer=opt_d)
    net_e = copy.deepcopy(base)
    opt_e = torch.optim.AdamW(groups(net_e), lr=LR, weight_decay=WD)
    st_e = train_step.CapturedStep(net_e, criterion, {"point_clouds": pool[0]})
    pe = list(net_e.parameters())
    assert st_d.launch == st_e.launch == "hipGraph replay"
    count = {"d": 0, "e": 0}

    def run_d():
        count["d"] += 1
        st_d.step(None, None, next_inputs=pool[count["d"] % len(pool)])
    cases["d_replay_with_fused_adamw_inside"] = run_d

    def run_e():
        count["e"] += 1
        st_e.step(None, None, next_inputs=pool[count["e"] % len(pool)])
        torch.nn.utils.clip_grad_norm_(pe, CLIP)
        opt_e.step()
    cases["e_replay_then_torch_adamw_clip"] = run_e

    net_f = copy.deepcopy(base)
    opt_f = optim.FusedAdamW(groups(net_f), lr=LR, weight_decay=WD, max_norm=CLIP, accum_steps=2)
    st_f = train_step.CapturedStep(net_f, criterion, {"point_clouds": pool[0]}, optimizer=opt_f, step_freq=2)
    net_g = copy.deepcopy(base)
    opt_g = optim.FusedAdamW(groups(net_g), lr=LR, weight_decay=WD, max_norm=CLIP)
    st_g = train_step.CapturedStep(net_g, criterion, {"point_clouds": pool[0]})
    assert st_f.launch == st_g.launch == "hipGraph replay"
    count.update(f=0, g=0)
    host_sum = {}

    def run_f():
        count["f"] += 1
        st_f.step(None, None, next_inputs=pool[count["f"] % len(pool)])
    cases["f_replay_accumulating_in_the_graph"] = run_f

    def run_g():
        count["g"] += 1
        st_g.step(None, None, next_inputs=pool[count["g"] % len(pool)])
        if "params" not in host_sum:
            host_sum["params"] = [p for p in net_g.parameters() if p.grad is not None]
            host_sum["sums"] = [torch.empty_like(p.grad) for p in host_sum["params"]]
        grads = [p.grad for p in host_sum["params"]]
        if count["g"] % 2:
            torch._foreach_copy_(host_sum["sums"], grads)
        else:
            torch._foreach_add_(host_sum["sums"], grads)
            for p, a in zip(host_sum["params"], host_sum["sums"]):
                p.grad = a                            # (the next replay hands the graph's own gradient tensors back)
            opt_g.step()
    cases["g_replay_accumulating_from_the_host"] = run_g

    # ---- the mean teacher: averaging inside the optimiser's launches (h, j) against the separate launch (i, k) --------------
    import ema
    EMA_DECAY = 0.999

    def teacher_of(net):
        t = copy.deepcopy(net)
        for p in t.parameters():
            p.requires_grad_(False)
            p.grad = None
        return t

    net_h = with_static_grads(copy.deepcopy(base))
    teacher_h = teacher_of(net_h)
    opt_h = optim.FusedAdamW(groups(net_h), lr=LR, weight_decay=WD, max_norm=CLIP)
    opt_h.attach_teacher(net_h, teacher_h, EMA_DECAY)
    cases["h_fused_adamw_with_teacher_eager"] = opt_h.step
    net_i = with_static_grads(copy.deepcopy(base))
    teacher_i = teacher_of(net_i)
    opt_i = optim.FusedAdamW(groups(net_i), lr=LR, weight_decay=WD, max_norm=CLIP)
    count.update(i=0, j=0, k=0)

    def run_i():
        count["i"] += 1
        opt_i.step()
        ema.update_ema_variables(net_i, teacher_i, EMA_DECAY, count["i"])
    cases["i_fused_adamw_then_ema_update_eager"] = run_i

    net_j = copy.deepcopy(base)
    teacher_j = teacher_of(net_j).train()
    opt_j = optim.FusedAdamW(groups(net_j), lr=LR, weight_decay=WD, max_norm=CLIP)
    st_j = train_step.CapturedStep(net_j, criterion, {"point_clouds": pool[0]}, teacher=teacher_j, ema=EMA_DECAY, optimizer=opt_j,
                                   ema_in_step=True)
    net_k = copy.deepcopy(base)
    teacher_k = teacher_of(net_k).train()
    opt_k = optim.FusedAdamW(groups(net_k), lr=LR, weight_decay=WD, max_norm=CLIP)
    st_k = train_step.CapturedStep(net_k, criterion, {"point_clouds": pool[0]}, teacher=teacher_k, ema=EMA_DECAY, optimizer=opt_k)
    assert st_j.launch == st_k.launch == "hipGraph replay"

    def run_j():
        count["j"] += 1
        st_j.step(None, None, next_inputs=pool[count["j"] % len(pool)])
    cases["j_mean_teacher_replay_averaging_inside"] = run_j

    def run_k():
        count["k"] += 1
        st_k.step(None, None, next_inputs=pool[count["k"] % len(pool)])
        st_k.update_teacher(count["k"])
    cases["k_mean_teacher_replay_then_update_teacher"] = run_k

    walls = {k: [] for k in cases}
    for rnd in range(args.rounds):
        for name, fn in cases.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            walls[name].append((time.perf_counter() - t0) * 1e3 / args.iters)
            print(f"round {rnd} {name:40s} {walls[name][-1]:8.4f} ms wall per iteration", flush=True)
    assert opt_f.t == opt_g.t == count["f"] // 2 == count["g"] // 2, (opt_f.t, opt_g.t, count)
    assert opt_h.global_step == 1 + opt_h.t and opt_j.global_step == 1 + count["j"] == 1 + opt_j.t, (opt_h.t, opt_j.t, count)
    for name, opt in list(fused.items()) + [("d", opt_d), ("f", opt_f), ("g", opt_g), ("h", opt_h), ("i", opt_i), ("j", opt_j),
                                            ("k", opt_k)]:
        assert opt.skipped == 0, f"{name}: {opt.skipped} steps were skipped for a non-finite gradient norm -- not a measurement"
    assert torch.isfinite(st_d.static_loss).item() and torch.isfinite(st_e.static_loss).item()
    assert torch.isfinite(st_f.static_loss).item() and torch.isfinite(st_g.static_loss).item()
    assert torch.isfinite(st_j.static_loss).item() and torch.isfinite(st_k.static_loss).item()
    import pointnet2_utils
    pointnet2_utils._ext.fps_check()

    out = {"tool": "bench_optimizer", "device": torch.cuda.get_device_name(0), "parameters": nparam, "tensors": ntensor,
           "batch": args.batch, "points": args.points, "rounds": args.rounds, "iters_per_round": args.iters,
           "bytes_needed": 32 * nparam, "cases": {}}
    for name, v in walls.items():
        out["cases"][name] = {"wall_ms_median": round(statistics.median(v), 4), "wall_ms_min": round(min(v), 4),
                              "wall_ms_max": round(max(v), 4), "wall_ms_spread": round(max(v) - min(v), 4),
                              "wall_ms_rounds": [round(x, 4) for x in v], "kernel_ms": None}
        print(f"{name:40s} wall median {statistics.median(v):8.4f} ms, spread {max(v) - min(v):7.4f} ms", flush=True)

    def verdict(new, old):
        n, o = out["cases"][new], out["cases"][old]
        return {"new": new, "old": old, "gain_ms": round(o["wall_ms_median"] - n["wall_ms_median"], 4),
                "old_spread_ms": o["wall_ms_spread"],
                "holds": bool(o["wall_ms_median"] - n["wall_ms_median"] > o["wall_ms_spread"])}
    out["requirements"] = [verdict("c_fused_adamw_eager", "a_torch_adamw_clip"),
                           verdict("d_replay_with_fused_adamw_inside", "e_replay_then_torch_adamw_clip"),
                           verdict("f_replay_accumulating_in_the_graph", "g_replay_accumulating_from_the_host")]

    def not_slower(new, old):
        """the in-launch averaging must not be slower than the separate launch by more than the spread of the latter's rounds"""
        n, o = out["cases"][new], out["cases"][old]
        return {"new": new, "old": old, "gain_ms": round(o["wall_ms_median"] - n["wall_ms_median"], 4),
                "old_spread_ms": o["wall_ms_spread"],
                "holds": bool(n["wall_ms_median"] - o["wall_ms_median"] <= o["wall_ms_spread"])}
    out["not_slower"] = [not_slower("h_fused_adamw_with_teacher_eager", "i_fused_adamw_then_ema_update_eager"),
                         not_slower("j_mean_teacher_replay_averaging_inside", "k_mean_teacher_replay_then_update_teacher")]
    print(json.dumps(out), flush=True)           # (kept even if the profiler pass below does not come back)

    if not args.no_kernel_time:
        for name, fn in cases.items():
            ms = kernel_time_ms(fn, 5)
            out["cases"][name]["kernel_ms"] = None if ms is None else round(ms, 4)
            print(f"{name:40s} summed kernel time {'not measured' if ms is None else f'{ms:8.4f} ms'} per iteration", flush=True)
    need = 32 * nparam
    for name in fused:
        c = out["cases"][name]
        for key, t in (("wall", c["wall_ms_median"]), ("kernel", c["kernel_ms"])):
            if t:
                rate = need / (t * 1e-3)
                c[f"{key}_bytes_per_s"] = round(rate, 0)
                c[f"{key}_fraction_of_8_TBps"] = round(rate / 8e12, 4)
                c[f"{key}_fraction_of_6.25_TBps_copy_ceiling"] = round(rate / 6.25e12, 4)
                print(f"{name:40s} {need / 1e6:.0f} MB / {key} time = {rate / 1e12:.3f} TB/s = {rate / 8e12:.1%} of 8 TB/s, "
                      f"{rate / 6.25e12:.1%} of the 6.25 TB/s copy ceiling", flush=True)
    # the averaging inside the launches (h: the norm reads g, the update reads p, g, m, v, e and writes p, m, v, e) and as a
    # fourth launch (i: 32 bytes as in (c), then e and p read and e written)
    for name, per_param in (("h_fused_adamw_with_teacher_eager", 36), ("i_fused_adamw_then_ema_update_eager", 40)):
        c = out["cases"][name]
        c["bytes_needed"] = per_param * nparam
        for key, t in (("wall", c["wall_ms_median"]), ("kernel", c["kernel_ms"])):
            if t:
                rate = per_param * nparam / (t * 1e-3)
                c[f"{key}_bytes_per_s"] = round(rate, 0)
                c[f"{key}_fraction_of_6.25_TBps_copy_ceiling"] = round(rate / 6.25e12, 4)
                print(f"{name:40s} {per_param * nparam / 1e6:.0f} MB ({per_param} B per parameter) / {key} time = "
                      f"{rate / 1e12:.3f} TB/s = {rate / 6.25e12:.1%} of the 6.25 TB/s copy ceiling", flush=True)
    if not args.no_kernel_time:
        # the accumulate launch alone, on a non-first micro-batch: 12 bytes per parameter
        net_acc = with_static_grads(copy.deepcopy(base))
        opt_acc = optim.FusedAdamW(groups(net_acc), lr=LR, weight_decay=WD, max_norm=CLIP, accum_steps=10 ** 6)
        for _ in range(args.warmup):
            opt_acc.step()
        ms = kernel_time_ms(opt_acc.step, 20, match="adamw_grad_sqnorm_kernel")
        assert opt_acc.t == 0 and 0 < opt_acc.micro < 10 ** 6
        acc = {"bytes_needed": 12 * nparam, "kernel_ms": None if ms is None else round(ms, 4)}
        if ms:
            rate = 12 * nparam / (ms * 1e-3)
            acc.update(bytes_per_s=round(rate, 0), fraction_of_8_TBps=round(rate / 8e12, 4),
                       **{"fraction_of_6.25_TBps_copy_ceiling": round(rate / 6.25e12, 4)})
            print(f"{'accumulate launch (accum_sqnorm)':40s} {12 * nparam / 1e6:.0f} MB / {ms:.4f} ms kernel time = "
                  f"{rate / 1e12:.3f} TB/s = {rate / 8e12:.1%} of 8 TB/s, {rate / 6.25e12:.1%} of the 6.25 TB/s copy ceiling "
                  f"(beside it: the norm pass + update of c_fused_adamw_eager above, {32 * nparam / 1e6:.0f} MB)", flush=True)
        else:
            print("accumulate launch (accum_sqnorm): kernel time not measured", flush=True)
        out["accumulate_launch"] = acc
    kb, kc = out["cases"]["b_torch_adamw_fused_clip"]["kernel_ms"], out["cases"]["c_fused_adamw_eager"]["kernel_ms"]
    if kb and kc:
        out["torch_fused_kernel_time_beats_ours"] = bool(kb < kc)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
