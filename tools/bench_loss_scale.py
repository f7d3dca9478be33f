"""A/B of the replayed fp16 training step with a static and with a dynamic loss scale (one MI355X, one process):

    (s) CapturedStep(amp_dtype=float16, loss_scale=2^14, optimizer=FusedAdamW(...))            <- the yardstick: the route of
        bench.py --dtype fp16, whose code the dynamic scale does not touch
    (d) CapturedStep(amp_dtype=float16, loss_scale="dynamic", optimizer=FusedAdamW(..., loss_scaler=LossScaler(init_scale=2^14)))

at the shapes of BASELINE configs[4] (16 scenes x 80 000 points; --batch 8 --points 40000 are configs[1]'s).  Both steppers are
built and warmed up first; then the two take turns, round after round, each round `--steps` replays between two device events
with a synchronise on either side.  Round 0 is thrown away.  What is reported per variant: median, min, max and the spread
(max - min) of its own rounds -- repeated runs of the SAME variant -- and whether (d) is slower than (s) by more than (s)'s
spread.  The dynamic scale adds one scalar recurrence to a one-workgroup launch and changes no streaming launch, so the
expectation is no difference beyond that spread; the tool reports what it measures either way.

    python tools/bench_loss_scale.py [--batch 16 --points 80000 --rounds 9 --steps 30] [--out profiles/dynamic_loss_scale_ab.txt]

Prints the text it writes to --out; the last line is one JSON record.
"""
import argparse
import copy
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import torch  # noqa: E402

import bench  # noqa: E402
import optim  # noqa: E402
import synth  # noqa: E402
import train_step  # noqa: E402

LR, DECODER_LR, WD, CLIP = 1e-6, 1e-7, 5e-4, 0.1          # tools/bench_optimizer.py's: the weights barely move over the run
SCALE = 2.0 ** 14


def groups(net):
    return [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
            {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": DECODER_LR}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=9, help="measured rounds per variant (one more, the first, warms up)")
    ap.add_argument("--steps", type=int, default=30, help="replays per round")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dynamic_loss_scale_ab.txt"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: at least 5, the spread of a variant's own rounds is the yardstick")
    dev = torch.device("cuda", 0)
    from procedural import load_procedural
    base = load_procedural(bench.build_model(0)).to(dev).train()
    pool = [synth.make_clouds(100 + i, args.batch, args.points, kind="room").to(dev) for i in range(3)]

    def criterion(ep, labels):
        return bench.loss_of(ep)

    net_s, net_d = copy.deepcopy(base), copy.deepcopy(base)
    opt_s = optim.FusedAdamW(groups(net_s), lr=LR, weight_decay=WD, max_norm=CLIP)
    opt_d = optim.FusedAdamW(groups(net_d), lr=LR, weight_decay=WD, max_norm=CLIP,
                             loss_scaler=optim.LossScaler(init_scale=SCALE))
    steppers = {
        "static_2^14": train_step.CapturedStep(net_s, criterion, {"point_clouds": pool[0]}, amp_dtype=torch.float16,
                                               loss_scale=SCALE, optimizer=opt_s),
        "dynamic_from_2^14": train_step.CapturedStep(net_d, criterion, {"point_clouds": pool[0]}, amp_dtype=torch.float16,
                                                     loss_scale="dynamic", optimizer=opt_d)}
    opts = {"static_2^14": opt_s, "dynamic_from_2^14": opt_d}
    for name, st in steppers.items():
        assert st.launch == "hipGraph replay", (name, st.launch)
    count = {name: 0 for name in steppers}
    times = {name: [] for name in steppers}
    for r in range(args.rounds + 1):
        for name, st in steppers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                count[name] += 1
                st.step(None, None, next_inputs=pool[count[name] % len(pool)])
            e1.record()
            torch.cuda.synchronize()
            if r > 0:                                        # round 0 warms both variants up
                times[name].append(e0.elapsed_time(e1) / args.steps)
    import pointnet2_utils
    pointnet2_utils._ext.fps_check()

    rec = {"tool": "bench_loss_scale", "device": torch.cuda.get_device_name(0), "batch": args.batch, "points": args.points,
           "dtype": "fp16", "rounds": args.rounds, "steps_per_round": args.steps, "variants": {}}
    lines = [f"# python tools/bench_loss_scale.py --batch {args.batch} --points {args.points} --rounds {args.rounds} "
             f"--steps {args.steps}",
             f"# the replayed fp16 step ({args.batch} x {args.points} points, hipGraph replay, FusedAdamW inside), static loss scale "
             "2^14 against",
             f"# dynamic from 2^14, taking turns in one process: {args.rounds} measured rounds of {args.steps} replays each "
             "(one more round in front warms up),",
             "# device events around each round, a synchronise on either side.  spread = max - min of a variant's OWN rounds.",
             "ms per step: median (min .. max) spread"]
    for name, v in times.items():
        opt = opts[name]
        info = {"ms_rounds": [round(x, 4) for x in v], "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                "ms_max": round(max(v), 4), "ms_spread": round(max(v) - min(v), 4), "replays": count[name], "t": opt.t,
                "skipped": opt.skipped, "loss_finite": bool(torch.isfinite(steppers[name].static_loss).item()),
                "scale_at_end": opt.scale_value if opt.loss_scaler is not None else 1.0 / opt.grad_scale}
        rec["variants"][name] = info
        lines.append("  %-20s %8.4f (%.4f .. %.4f) %.4f    steps taken %d, skipped %d, scale at the end %g" %
                     (name, info["ms_median"], info["ms_min"], info["ms_max"], info["ms_spread"], info["t"], info["skipped"],
                      info["scale_at_end"]))
    s, d = rec["variants"]["static_2^14"], rec["variants"]["dynamic_from_2^14"]
    diff = round(d["ms_median"] - s["ms_median"], 4)
    rec["dynamic_minus_static_ms"] = diff
    rec["slower_than_the_static_routes_own_spread"] = bool(diff > s["ms_spread"])
    lines.append(f"dynamic - static = {diff:+.4f} ms ({100.0 * diff / s['ms_median']:+.2f} %); the static route's own spread is "
                 f"{s['ms_spread']:.4f} ms, the dynamic route's {d['ms_spread']:.4f} ms")
    if rec["slower_than_the_static_routes_own_spread"]:
        lines.append("-> the dynamic step is SLOWER than the static one by more than the static route's spread of repeated runs")
    else:
        lines.append("-> no difference beyond the spread of repeated runs of the static route")
    if s["skipped"] != d["skipped"]:
        lines.append(f"   (the two variants did not skip the same number of steps: {s['skipped']} and {d['skipped']} -- a skipped step "
                     "runs the same launches, whose update returns early)")
    lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
