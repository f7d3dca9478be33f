#!/usr/bin/env python
"""What the two host lines left in the reference's training loop cost per step, and what is left of that cost with both on
the device: `scheduler.step()` (train.py:566) and the stat_dict loop with its `.item()` per key (train.py:580-586).

The workload is bench.py --mean-teacher's (PQ_Transformer, bf16, batch 8, 40 000-point rooms, the step replayed from a
hipGraph), the batch read as 4 labelled + 4 unlabelled scenes, criterion semi_objective.SemiSupervisedObjective, clip + AdamW
and the teacher's averaging inside the captured step (optimizer=FusedAdamW, ema_in_step=True).  Three steppers live in one
process and take turns inside every round:

    (floor)   no scheduler, no reads: `stepper.step(...)` and nothing else
    (host)    torch's CosineAnnealingLR stepped on the host every step (it writes param_groups, the stepper stages the rows),
              and `.item()` on every key of objective.stats that train.py:581 selects, plus the gradient norm -- the
              reference's loop as it stands
    (device)  FusedAdamW(lr_schedule=LRSchedule(...)) and CapturedStep(stats=lambda: objective.stats); one stats.read() per
              `--print-freq` steps

A sample is the WALL time of `--steps` steps between two device synchronisations (host reads are what is measured, so device
events would miss the point); `--rounds` rounds, one short unmeasured sample per side in front.  Reported per side: the
median ms per step and the spread (max - min) of its own samples, and the number of selected keys.

    python tools/bench_train_loop.py [--steps 200] [--rounds 5] [--print-freq 10] [--out profiles/train_loop_ab.txt]

Writes --out whole and prints it; the last line is one JSON record.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

LR, DECODER_LR, WD, CLIP = 1e-6, 1e-7, 5e-4, 0.1          # tools/bench_optimizer.py's: the weights barely move over the run
B, HALF, POINTS = 8, 4, 40000


def groups(net):
    return [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
            {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": DECODER_LR}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="replayed steps per sample")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--print-freq", type=int, default=10, help="steps per stats.read() on the device side")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_loop_ab.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import mt_inputs
    import optim
    import semi_objective
    import step_stats
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    base = bench.build_model(0).to(dev).train()
    clouds = [synth.make_clouds(100 + i, B, POINTS, kind="room") for i in range(3)]
    pool = [c.to(dev) for c in clouds]
    teacher_pool = [synth.make_clouds(200 + i, B, POINTS, kind="room").to(dev) for i in range(3)]
    mean_size = bench.mean_size_arr()
    rng = np.random.default_rng(5)
    lab = synth.make_labels(clouds[0], 300, mean_size_arr=mean_size)
    size = mean_size[lab["size_class_label"].numpy()] + lab["size_residual_label"].numpy()
    normals = rng.standard_normal((HALF, POINTS, 3))
    labels = {k: v[:HALF].to(dev) for k, v in lab.items()}
    labels.update({"unlabeled.center_label": lab["center_label"][HALF:].to(dev),
                   "unlabeled.size_label": torch.from_numpy(size[HALF:].astype(np.float32)).to(dev),
                   "unlabeled.num_gt_boxes": lab["num_gt_boxes"][HALF:].to(dev),
                   "unlabeled.point_clouds": pool[0][HALF:, :, :3].contiguous(),
                   "unlabeled.vertex_normals": torch.from_numpy(
                       (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(np.float32)).to(dev),
                   "consistency_weight": torch.tensor(1.0, device=dev)})
    for k, v in mt_inputs.augmentation(rng, B).items():
        labels[k], labels["unlabeled." + k] = torch.from_numpy(v[:HALF]).to(dev), torch.from_numpy(v[HALF:]).to(dev)

    class DatasetConfig(bench.LossConfig):
        mean_size_arr = mean_size

    cfg = types.SimpleNamespace(pc_loss=True, gamma_mixture=True, ema=True, arkit=True, lambda_metric_normal=1.0,
                                lambda_metric_vertical=1.0, lambda_metric_size=1.0, lambda_metric_score=1.0,
                                lambda_arkit_pc_loss=1.0)
    total = args.steps * (args.rounds + 1)

    def build(side):
        net = copy.deepcopy(base)
        teacher = copy.deepcopy(base)
        for p in teacher.parameters():
            p.detach_()
        teacher.train()
        objective = semi_objective.SemiSupervisedObjective(DatasetConfig, cfg)
        sched = optim.LRSchedule("cosine", 1, total, -1) if side == "device" else None
        opt = optim.FusedAdamW(groups(net), lr=LR, weight_decay=WD, max_norm=CLIP, lr_schedule=sched)
        st = train_step.CapturedStep(net, objective, {"point_clouds": pool[0]}, labels, teacher=teacher,
                                     teacher_example={"point_clouds": teacher_pool[0]}, ema=bench.EMA_DECAY,
                                     teacher_to_criterion=True, warmup=3, optimizer=opt, ema_in_step=True,
                                     stats=(lambda: objective.stats) if side == "device" else None)
        assert st.launch == "hipGraph replay", (side, st.launch)
        host_sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=total + 1, eta_min=1e-6) if side == "host" else None
        return types.SimpleNamespace(side=side, st=st, opt=opt, objective=objective, host_sched=host_sched, count=0,
                                     stat_dict={}, reads=0, samples=[])

    sides = [build(s) for s in ("floor", "host", "device")]
    selected = len(step_stats.StepStats.select(sides[1].objective.stats)[0])

    def run(s, steps):
        st = s.st
        for _ in range(steps):
            s.count += 1
            i = s.count
            st.step(None, labels, next_inputs=pool[i % 3], next_teacher_inputs=teacher_pool[i % 3])
            if s.side == "host":
                s.host_sched.step()                                           # train.py:566
                s.stat_dict["grad_norm"] = s.opt.grad_total_norm.item()       # train.py:578 (logged through .item() at :593)
                s.reads += 1
                ep = s.objective.stats
                for key in ep:                                                # train.py:580-586
                    if "loss" in key or "acc" in key or "ratio" in key:
                        if key not in s.stat_dict:
                            s.stat_dict[key] = 0
                        s.stat_dict[key] += ep[key] if isinstance(ep[key], float) else ep[key].item()
                        s.reads += 1
            elif s.side == "device" and i % args.print_freq == 0:
                s.window = st.stats.read()
                s.reads += 1

    def sample(s, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(s, steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for s in sides:
        sample(s, 20)                                                         # unmeasured
    for _ in range(args.rounds):
        for s in sides:                                                       # the three sides alternate inside every round
            s.samples.append(sample(s, args.steps))
    import pointnet2_utils
    pointnet2_utils._ext.fps_check()

    rec = {"tool": "bench_train_loop", "device": torch.cuda.get_device_name(0), "batch": B, "points": POINTS,
           "steps_per_sample": args.steps, "rounds": args.rounds, "print_freq": args.print_freq, "selected_keys": selected,
           "sides": {}}
    lines = [f"# python tools/bench_train_loop.py --steps {args.steps} --rounds {args.rounds} --print-freq {args.print_freq}",
             f"# the replayed mean-teacher step (bench.py --mean-teacher's workload: {B} x {POINTS} points, bf16, 4 labelled + 4",
             "# unlabelled scenes, criterion SemiSupervisedObjective, clip + AdamW + teacher averaging inside the captured step),",
             f"# three steppers in one process taking turns inside every round; a sample = wall time of {args.steps} steps between two",
             f"# device synchronisations; {args.rounds} rounds.  spread = max - min of a side's OWN samples.",
             f"# keys of objective.stats selected by train.py:581's rule: {selected} (+ grad_norm)",
             "ms per step: median (min .. max) spread"]
    for s in sides:
        v = s.samples
        info = {"ms_samples": [round(x, 4) for x in v], "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                "ms_max": round(max(v), 4), "ms_spread": round(max(v) - min(v), 4), "steps": s.count, "host_reads": s.reads,
                "staged": s.opt.staged, "t": s.opt.t, "skipped": s.opt.skipped}
        rec["sides"][s.side] = info
        lines.append("  %-8s %8.4f (%.4f .. %.4f) %.4f    host reads %d, hyper-parameter rows staged %d times, steps taken %d" %
                     (s.side, info["ms_median"], info["ms_min"], info["ms_max"], info["ms_spread"], s.reads, s.opt.staged,
                      info["t"]))
    f, h, d = (rec["sides"][k] for k in ("floor", "host", "device"))
    rec["device_minus_floor_ms"] = round(d["ms_median"] - f["ms_median"], 4)
    rec["host_minus_floor_ms"] = round(h["ms_median"] - f["ms_median"], 4)
    rec["device_within_the_floors_spread"] = bool(abs(rec["device_minus_floor_ms"]) <= f["ms_spread"])
    rec["host_slower_than_the_floors_spread"] = bool(rec["host_minus_floor_ms"] > f["ms_spread"])
    lines.append(f"device - floor = {rec['device_minus_floor_ms']:+.4f} ms, host - floor = {rec['host_minus_floor_ms']:+.4f} ms; the "
                 f"floor's own spread over the {args.rounds} rounds is {f['ms_spread']:.4f} ms")
    lines.append("-> the device side lies " + ("WITHIN" if rec["device_within_the_floors_spread"] else "OUTSIDE") +
                 " the floor's own spread; the host side is " +
                 ("slower than the floor by MORE than that spread" if rec["host_slower_than_the_floors_spread"]
                  else "NOT slower than the floor by more than that spread"))
    last = sides[2].window
    lines.append(f"   (device side, last window: {last.steps} steps, total_loss mean {last.means()['total_loss']:.6g}, grad_norm "
                 f"{last['grad_norm']:.6g}; lr now {sides[2].opt.lr_schedule.get_last_lr()})")
    lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
