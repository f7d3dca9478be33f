"""A/B of the input side of the mean-teacher step (one MI355X, a process of its own):

    python tools/bench_assemble.py [--out profiles/assemble_ab.txt]

  device   SceneBank.assemble of a 16-cloud mean-teacher batch -- 8 labelled + 8 unlabelled items, scenes of 150 000 rows ->
           40 000 points, device draw, static output buffers, the four augmentation numbers per item drawn on the host and
           uploaded: 4 + 2 launches.  Device events around the calls, then a synchronise.
  host     the same 16 items by the numpy restatement of the datasets' `__getitem__` (tests/assemble_restatement.py, with the
           reference's np.random.choice draws) in 16 worker processes, collated, copied to pinned memory and on to the device:
           what a DataLoader with 16 workers delivers at best, with a scene's static parts kept per worker.  Wall clock to the
           synchronise after the copy.
  step     the replayed mean-teacher step of `bench.py --gpus 1 --mean-teacher` and plain `bench.py --gpus 1`, run as child
           processes before the two sides; the host side's time per item on one core is taken in this process.

The two sides alternate round by round after a warm-up; median and (min .. max) of the rounds are reported.  The file is
written whole, explanatory header included; `--step` (run it second) appends the blocks that are not a gate: the replayed
default step fed three ways, and eager steps fed by a DeviceLoader without and with `net=`.
"""
import argparse
import json
import multiprocessing
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "omni-pq_amd"), os.path.join(REPO, "omni-pq_amd", "pointnet2"),
          os.path.join(REPO, "omni-pq_amd", "models")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROWS, POINTS, LABELLED, UNLABELLED = 150000, 40000, 8, 8


def labelled_scene(i, rows=ROWS):
    """as tests/assemble_inputs.py builds them, at the dataset's size: 30 instances, 20 boxes"""
    import assemble_inputs as A
    rs = np.random.RandomState(500 + i)
    n_inst, n_box = 30, 20
    owner = rs.randint(0, n_inst, size=rows)
    centre = rs.rand(n_inst, 3) * [6.0, 5.0, 2.0] - [3.0, 2.5, 0.0]
    xyz = (centre[owner] + 0.25 * rs.randn(rows, 3)).astype(np.float32)
    nrm = rs.randn(rows, 3).astype(np.float32)
    sem_of = np.where(rs.rand(n_inst) < 0.7, rs.choice(A.NYU40IDS, n_inst), 1)
    ang = rs.rand(8) * 2 * np.pi
    return {"vertices": np.concatenate([xyz, rs.randint(0, 256, size=(rows, 3)).astype(np.float32)], 1), "normals": nrm,
            "instance_labels": owner.astype(np.int64) * 3 + 1, "semantic_labels": sem_of[owner].astype(np.int64),
            "boxes": np.concatenate([centre[:n_box] + 0.1 * rs.randn(n_box, 3), 0.3 + 1.2 * rs.rand(n_box, 3),
                                     rs.choice(A.NYU40IDS, n_box)[:, None].astype(np.float64)], 1),
            "rectangles": np.concatenate([rs.rand(8, 3) * [6.0, 5.0, 0.0] + [-3.0, -2.5, 1.3],
                                          np.stack([np.cos(ang), np.sin(ang), np.zeros(8)], 1), 1.0 + 3.0 * rs.rand(8, 1),
                                          np.full((8, 1), 2.6)], 1),
            "total_quad_num": 10, "horizontal_quads": rs.rand(2, 4, 3) * [6.0, 5.0, 2.6] - [3.0, 2.5, 0.0]}


def unlabelled_scene(i, rows=ROWS):
    rs = np.random.RandomState(900 + i)
    return {"vertices": (rs.rand(rows, 3) * [6.0, 5.0, 2.6] - [3.0, 2.5, 0.2]).astype(np.float32),
            "normals": rs.randn(rows, 3).astype(np.float32),
            "boxes": np.concatenate([rs.rand(10, 3) * [6.0, 5.0, 2.0] - [3.0, 2.5, 0.0], 0.3 + rs.rand(10, 3),
                                     rs.rand(10, 1) * 2 * np.pi], 1)}


# ---- host side: one item per task, in worker processes that never open the GPU ---------------------------------------------
_cache = {}


def host_item(task):
    import assemble_inputs as A
    import assemble_restatement as R
    kind, i, seed = task
    if (kind, i) not in _cache:
        sc = labelled_scene(i) if kind == 0 else unlabelled_scene(i)
        _cache[(kind, i)] = (sc, R.static_scannet(sc) if kind == 0 else R.static_arkit(sc))
    sc, static = _cache[(kind, i)]
    rs = np.random.RandomState(seed)
    n = sc["vertices"].shape[0]
    ema, choices = rs.choice(n, POINTS, replace=n < POINTS), rs.choice(n, POINTS, replace=n < POINTS)
    angle = (rs.random_sample() * np.pi / 18) - np.pi / 36 + rs.randint(4) * np.pi / 2
    c, s = np.cos(angle), np.sin(angle)
    params = (rs.random_sample() > 0.5, rs.random_sample() > 0.5, np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]),
              rs.random_sample() * 0.3 + 0.85)
    if kind == 0:
        out = R.scannet_item(sc, A.Config, choices, ema, params, slot=i, static=static)
        del out["argmin_margins"]
    else:
        out = R.arkit_item(sc, choices, ema, params, static=static)
    return out


def host_batch(pool, round_no, torch, pinned):
    """16 items from the workers -> collated -> pinned -> device; -> seconds"""
    tasks = [(0, i, 1000 * round_no + i) for i in range(LABELLED)] + [(1, i, 1000 * round_no + 100 + i) for i in range(UNLABELLED)]
    t0 = time.perf_counter()
    items = pool.map(host_item, tasks, chunksize=1)
    dev = []
    for which, group in enumerate((items[:LABELLED], items[LABELLED:])):
        for key in group[0]:
            arr = np.stack([it[key] for it in group])
            slot = pinned.setdefault((which, key), torch.empty(arr.shape, dtype=torch.from_numpy(arr).dtype, pin_memory=True))
            slot.copy_(torch.from_numpy(arr))
            dev.append(slot.to("cuda", non_blocking=True))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def step_reference(steps, warmup, *flags):
    """`bench.py --gpus 1 [--mean-teacher]` in a child process -> its JSON record"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *flags, "--steps", str(steps),
                          "--warmup", str(warmup)], capture_output=True, text=True, timeout=420)
    if out.returncode != 0:
        raise RuntimeError(f"bench.py {' '.join(flags)} failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


HEADER = """# The input side of the mean-teacher step, device against host (one MI355X, one session; written by this tool, header included).
#   device   SceneBank.assemble of the 16-cloud batch (8 labelled + 8 unlabelled items, scenes of 150 000 rows -> 40 000 points,
#            device draw, static output buffers, parameters drawn on the host and uploaded): 4 + 2 launches
#   host     the same 16 items by the numpy restatement of the datasets' __getitem__ (tests/assemble_restatement.py) in worker
#            processes, collated, through pinned memory to the device; the per-item line is one core of the same machine
#   step     bench.py --gpus 1 --mean-teacher and plain bench.py --gpus 1, child processes of the same run
# Acceptance: the device batch takes less time than the host side and less than one replayed mean-teacher step (last line
# of the first block).  `--step` appends the second block, which is not a gate: bench.py's replayed default step with the next
# batch handed over as `next_inputs` from a resident tensor, from a DeviceLoader assembling on a stream of its own and from a
# DeviceLoader assembling on the training stream between replays; then eager steps fed by the loader without and with net=.
"""


def one_core_ms():
    """ms per item of the host side on one core of this machine, in this process: (labelled, unlabelled)"""
    out = []
    for kind in (0, 1):
        host_item((kind, 0, 1))                              # builds the scene and its static parts
        t = []
        for seed in (2, 3, 4):
            t0 = time.perf_counter()
            host_item((kind, 0, seed))
            t.append(time.perf_counter() - t0)
        out.append(1e3 * sorted(t)[1])
    return out


def fed_step(steps, rounds, out):
    """`python bench.py`'s replayed default step (batch 8, 40 000 points, bf16) with the NEXT batch handed over as
    `next_inputs` three ways, taking turns: a resident tensor of the pool (what bench.py times), a DeviceLoader batch assembled
    on the loader's own stream, a DeviceLoader batch assembled on the training stream between replays."""
    import torch
    import synth
    import bench
    import assemble_inputs as A
    import device_data as D
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        args = bench.parse()
    finally:
        sys.argv = argv
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    net = bench.build_model(0).to(dev)
    net.train()
    pool = [synth.make_clouds(100 + i, args.batch, args.points, kind="room").to(dev) for i in range(3)]
    args.feeder = None
    bench.make_step(net, net, pool, args, torch.bfloat16, 1)
    stepper = args.stepper
    bank = D.SceneBank(dev, A.Config, use_height=False, seed=3)
    for i in range(2 * args.batch):
        sc = labelled_scene(i)
        bank.add_scene(f"l{i}", sc["vertices"], sc["normals"], sc["instance_labels"], sc["semantic_labels"], sc["boxes"],
                       sc["rectangles"], sc["total_quad_num"], sc["horizontal_quads"])

    class Feed:
        def __init__(self, side_stream):
            self.loader = D.DeviceLoader(bank, args.batch, seed=0, num_points=args.points, side_stream=side_stream)
            self.epoch, self.it = 0, None

        def __call__(self, dst):
            batch = None if self.it is None else next(self.it, None)
            if batch is None:
                self.loader.sampler.set_epoch(self.epoch)
                self.epoch += 1
                self.it = iter(self.loader)
                batch = next(self.it)
            dst.copy_(batch["point_clouds"])

    count = [0]

    def resident():
        count[0] += 1
        return pool[count[0] % len(pool)]

    feeds = {"resident tensor": resident, "DeviceLoader, own stream": Feed(True), "DeviceLoader, training stream": Feed(False)}
    times = {name: [] for name in feeds}
    for r in range(rounds + 1):
        for name, feed in feeds.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                stepper.step(None, None, next_inputs=feed() if feed is resident else feed)
            e1.record()
            torch.cuda.synchronize()
            if r > 0:                                        # round 0 warms every variant up
                times[name].append(e0.elapsed_time(e1) / steps)
    lines = [f"# python tools/bench_assemble.py --step        (bench.py's replayed default step, batch {args.batch} x {args.points} "
             f"points, {stepper.launch}; the next batch handed over three ways, taking turns: {rounds} rounds of {steps} steps)",
             "ms per step, median (min .. max)"]
    rec = {}
    for name, v in times.items():
        v = sorted(v)
        rec[name] = v
        lines.append("  %-32s %8.3f (%.3f .. %.3f)" % (name, v[len(v) // 2], v[0], v[-1]))
    lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    with open(out, "a") as fh:
        fh.write("\n" + text)
    lines = []

    # the loader's net= : eager forward + backward of a second network (bf16 autocast, bench.py's loss) on the loader's batches,
    # with and without the loader announcing every batch to the backbone's sampling prefetch as it hands it out
    net2 = bench.build_model(0).to(dev)
    net2.train()

    def eager(loader, steps):
        done, epoch = 0, 0
        while done < steps:
            loader.sampler.set_epoch(epoch)
            epoch += 1
            for batch in loader:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = bench.loss_of(net2({"point_clouds": batch["point_clouds"]}))
                loss.backward()
                for q in net2.parameters():
                    q.grad = None
                done += 1

    loaders = {"DeviceLoader": D.DeviceLoader(bank, args.batch, seed=0, num_points=args.points),
               "DeviceLoader, net=": D.DeviceLoader(bank, args.batch, seed=0, num_points=args.points, net=net2)}
    etimes = {name: [] for name in loaders}
    esteps = max(4, steps // 3)
    for r in range(rounds + 1):
        for name, loader in loaders.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            eager(loader, esteps)
            e1.record()
            torch.cuda.synchronize()
            if r > 0:
                etimes[name].append(e0.elapsed_time(e1) / esteps)
    lines.append(f"eager forward + backward fed by the loader (batch {args.batch} x {args.points} points, bf16), ms per step, median "
                 f"(min .. max) of {rounds} rounds of {esteps} steps")
    erec = {}
    for name, v in etimes.items():
        v = sorted(v)
        erec[name] = v
        lines.append("  %-32s %8.3f (%.3f .. %.3f)" % (name, v[len(v) // 2], v[0], v[-1]))
    lines.append(json.dumps(erec))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "a") as fh:
        fh.write("\n" + text)


def main():
    if "--step" in sys.argv:
        ap = argparse.ArgumentParser()
        ap.add_argument("--step", action="store_true")
        ap.add_argument("--steps", type=int, default=30)
        ap.add_argument("--rounds", type=int, default=5)
        ap.add_argument("--out", default=os.path.join(REPO, "profiles", "assemble_ab.txt"))
        a = ap.parse_args()
        return fed_step(a.steps, a.rounds, a.out)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--step-steps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "assemble_ab.txt"))
    args = ap.parse_args()

    step = None if args.no_step else step_reference(args.step_steps, 3, "--mean-teacher")
    plain = None if args.no_step else step_reference(50, 3)
    per_item = one_core_ms()
    pool = multiprocessing.get_context("spawn").Pool(args.workers)       # started before this process opens the GPU
    pool.map(host_item, [(0, i, 1) for i in range(LABELLED)] + [(1, i, 1) for i in range(UNLABELLED)], chunksize=1)

    import torch
    import assemble_inputs as A
    import device_data as D
    lab, unl = D.SceneBank("cuda", A.Config, seed=1), D.SceneBank("cuda", seed=2)
    for i in range(LABELLED):
        sc = labelled_scene(i)
        lab.add_scene(f"l{i}", sc["vertices"], sc["normals"], sc["instance_labels"], sc["semantic_labels"], sc["boxes"],
                      sc["rectangles"], sc["total_quad_num"], sc["horizontal_quads"])
    for i in range(UNLABELLED):
        sc = unlabelled_scene(i)
        unl.add_unlabelled_scene(f"u{i}", sc["vertices"], sc["normals"], sc["boxes"])
    bufs = (lab.make_buffers(LABELLED, POINTS), unl.make_buffers(UNLABELLED, POINTS))
    slots = (list(range(LABELLED)), list(range(UNLABELLED)))

    def device_batch():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for bank, buf, sl in zip((lab, unl), bufs, slots):
            bank.assemble(sl, num_points=POINTS, out=buf)
            bank.seed.add_(1)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0

    pinned = {}
    dev_ev, dev_wall, host = [], [], []
    for r in range(args.warmup + args.rounds):
        d = device_batch()
        h = host_batch(pool, r, torch, pinned)
        if r >= args.warmup:
            dev_ev.append(d[0])
            dev_wall.append(d[1])
            host.append(h)
    pool.close()
    pool.join()
    mask = bufs[0]["vote_label_mask"]
    distinct = int(torch.unique(bufs[0]["choices"][0]).numel())

    def stat(v):
        v = sorted(v)
        return 1e3 * v[len(v) // 2], 1e3 * v[0], 1e3 * v[-1]

    lines = [f"# python tools/bench_assemble.py        (one MI355X; a process of its own; device and host side alternate, "
             f"{args.rounds} rounds after {args.warmup} warm-up rounds)",
             f"16-cloud mean-teacher batch: {LABELLED} labelled + {UNLABELLED} unlabelled items, {ROWS} rows -> {POINTS} points; "
             "ms per batch, median (min .. max)",
             "  device, events       %8.3f (%.3f .. %.3f)    SceneBank.assemble x 2 (4 + 2 launches), device draw" % stat(dev_ev),
             "  device, wall clock   %8.3f (%.3f .. %.3f)    the same calls from Python to the synchronise" % stat(dev_wall),
             f"  host, {args.workers} workers     %8.3f (%.3f .. %.3f)    restatement of __getitem__ per item + collate + pinned copy"
             % stat(host),
             f"  (labelled rows that vote in the last batch: {float(mask.float().mean()):.3f}; distinct rows in scene 0's draw: "
             f"{distinct} of {POINTS})"]
    lines.append("  host, one core, one item   labelled %.1f ms, unlabelled %.1f ms (median of three, this process)" % tuple(per_item))
    rec = {"host_item_ms": per_item, "device_event_ms": stat(dev_ev), "device_wall_ms": stat(dev_wall), "host_ms": stat(host), "rounds": args.rounds,
           "workers": args.workers, "rows": ROWS, "points": POINTS}
    if step is not None:
        lines.append("  replayed mean-teacher step (bench.py --gpus 1 --mean-teacher --steps %d): %.3f ms per step, median %.3f, "
                     "p10 .. p90 %.3f .. %.3f" % (args.step_steps, step["ms_per_step"], step["median_ms_per_step"],
                                                 *step.get("p10_p90_ms_per_step", [float("nan")] * 2)))
        rec["step_ms"] = step["ms_per_step"]
        rec["step_median_ms"] = step["median_ms_per_step"]
        lines.append("  device batch / step = %.3f; device batch / host batch = %.4f" %
                     (stat(dev_wall)[0] / step["median_ms_per_step"], stat(dev_wall)[0] / stat(host)[0]))
    if plain is not None:
        lines.append("  python bench.py --gpus 1 --steps 50 --warmup 3 (no code of the input side on its path): %.3f ms per step, "
                     "median %.3f" % (plain["ms_per_step"], plain["median_ms_per_step"]))
        rec["bench_ms"] = plain["ms_per_step"]
    lines.append(json.dumps(rec))
    text = HEADER + "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
