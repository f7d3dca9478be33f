#!/usr/bin/env python
"""A/B of the scoring tail of an evaluation pass -- from the captured forward to the layout F1 of the pass -- on the benchmark
model in eval mode under bf16 autocast:

    (a) parent   per batch CapturedInference.run() (which queues the record's device-to-host copy), to_lists(),
                 parse_quad_groundtruths for the ground-truth lists, QUADAPCalculator.step; compute_F1 for both values of
                 `calculated` at the end.  The route before csrc/layout_f1.hip, unchanged in this tree.
    (b) device   inference.evaluate_layout_f1 (run(to_host=False) + LayoutF1.step per batch) and ONE read() at the end; both F1
                 values from the five integers.

    python tools/bench_layout_f1.py [--points 40000] [--batches 8 1] [--passes 12] [--rounds 5] [--out profiles/layout_f1_ab.txt]

A sample is one pass over `passes` batches (clouds and synthetic quad labels of synth.make_labels, on the device) timed on the
host clock, ending with the F1 values in Python floats.  Both routes replay the same captured graph (quads of `last_` only) and
announce the next batch; they alternate inside every round (same process, same inputs); the table reports the median over the
rounds and the spread (max - min) next to it, and calls route (b) faster only where its median is below the parent's by more
than the two spreads together.  The two routes must agree on both F1 values bit for bit before anything is timed."""
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
from bench_inference import DatasetConfig  # noqa: E402

LABELS = ("gt_quad_centers", "gt_normal_vectors", "gt_quad_sizes", "num_gt_quads", "num_total_quads", "horizontal_quads")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--passes", type=int, default=12, help="batches per evaluation pass")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layout_f1_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layout_f1: needs a GPU (nothing is timed without one)")
    import ap_helper_pq
    import inference
    import synth
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = bench.build_model(0).to(dev).eval()
    cfg = {"remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
           "per_class_proposal": True, "conf_thresh": 0.0, "dataset_config": DatasetConfig()}     # the reference's eval.py
    lines = [f"# python tools/bench_layout_f1.py --points {args.points} --batches {' '.join(map(str, args.batches))} "
             f"--passes {args.passes} --rounds {args.rounds}        ({torch.cuda.get_device_name(0)}, one process)",
             "# eval / bf16, one evaluation pass from the captured forward to both layout F1 values; ms per batch: median over "
             "the rounds (spread = max - min); the two routes alternate inside every round"]
    for B in args.batches:
        pool = []
        for i in range(3):
            pc = synth.make_clouds(100 + i, B, args.points, kind="room")
            labels = synth.make_labels(pc, 200 + i)
            batch = {k: labels[k].to(dev) for k in LABELS}
            batch["point_clouds"] = pc.to(dev)
            pool.append(batch)
        epoch = [pool[i % 3] for i in range(args.passes)]
        runner = inference.CapturedInference(net, pool[0], cfg, objects=False)
        assert runner.launch == "hipGraph replay"

        def parent():
            calc = ap_helper_pq.QUADAPCalculator(0.25, {1: "quad"})
            for i, batch in enumerate(epoch):
                nxt = epoch[i + 1] if i + 1 < len(epoch) else None
                quads = runner.run(batch, next_inputs=nxt)["last_"][1]
                pred_map, _, corners = quads.to_lists()
                gt_map, gt_corners = ap_helper_pq.parse_quad_groundtruths(batch, cfg)
                calc.step(pred_map, gt_map, corners, gt_corners, batch["horizontal_quads"])
            return calc.compute_F1(calculated=False), calc.compute_F1(calculated=True)

        def device():
            counts = inference.evaluate_layout_f1(runner, epoch).read()
            return ap_helper_pq.f1_from_counts(counts, False), ap_helper_pq.f1_from_counts(counts, True)

        routes = {"parent": parent, "device": device}
        want = parent()
        runner.forget_next()
        got = device()
        assert got == want, (got, want)                       # the same number, bit for bit, before anything is timed
        counts = inference.evaluate_layout_f1(runner, epoch).read()
        lines.append(f"# batch {B}: counts of one pass {counts}; F1 {want[0]:.6f}, with the deduced ceiling and floor {want[1]:.6f}")
        t = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                runner.forget_next()
                fn()                                          # warm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / len(epoch) * 1e3)
        med = {n: statistics.median(v) for n, v in t.items()}
        spr = {n: max(v) - min(v) for n, v in t.items()}
        for name in routes:
            verdict = ""
            if name != "parent":
                faster = med[name] < med["parent"] - (spr[name] + spr["parent"])
                verdict = f"   parent / this {med['parent'] / med[name]:5.2f}   " + \
                    ("faster than the parent" if faster else "not faster beyond the spreads")
            lines.append(f"batch {B} {name:7s} {med[name]:8.3f} ms ({spr[name]:.3f})   {B / med[name] * 1e3:8.1f} scenes/s{verdict}")
        del runner
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
