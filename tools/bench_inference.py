#!/usr/bin/env python
"""A/B of one evaluation batch, forward to host lists, on the benchmark model in eval mode under bf16 autocast:

    (a) parent    eager forward + ap_helper_pq.parse_predictions + parse_quad_predictions (the route before DESIGN 4.11)
    (b) eager+L1  eager forward + detect_predictions + detect_quad_predictions + to_lists  (inference.CapturedInference(graph=False))
    (c) replay    the same body replayed as one graph + to_lists                           (inference.CapturedInference)

    python tools/bench_inference.py [--points 40000] [--batches 8 1] [--rounds 5] [--iters 30] [--out profiles/inference_ab.txt]

Each sample is `iters` batches timed on the host clock, every batch ending with its Python lists built (which waits for the
readback), so all three routes deliver the same thing; (b) and (c) announce the next batch, as an evaluation loop would.  The
three routes alternate inside every round (same process, same inputs); the table reports the median over the rounds and the
spread (max - min) next to it, and calls a route faster than the parent only where its median is below the parent's by more
than the two spreads together.  Next to the times: what follows the forward on routes (a) and (b), counted once -- ATen GPU
ops and C-ABI launches (a TorchDispatchMode and a counter around pointnet2._ext._run) and device-to-host copies."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import bench  # noqa: E402

_VIEWS = {"view", "_unsafe_view", "transpose", "t", "slice", "select", "unsqueeze", "squeeze", "expand", "as_strided", "detach",
          "alias", "permute", "reshape", "empty", "empty_like", "empty_strided", "split", "split_with_sizes", "unbind", "narrow",
          "_reshape_alias", "view_as", "lift_fresh", "chunk", "record_stream", "is_same_size", "contiguous", "_pin_memory",
          "is_pinned"}


class DatasetConfig:
    """what the parse functions read of a ScanNet-style dataset config, with the benchmark model's class means"""
    num_class = 18
    num_heading_bin = 1
    num_size_cluster = 18

    def __init__(self):
        self.mean_size_arr = np.asarray(bench.mean_size_arr(), dtype=np.float64)

    def class2angle(self, pred_cls, residual, to_label_format=True):
        return 0


class Count(TorchDispatchMode):
    """ATen ops that produce a GPU tensor (views excluded), and copies that land on the host"""

    def __init__(self):
        super().__init__()
        self.aten = self.d2h = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        base = str(func).split(".")[1] if "." in str(func) else str(func)
        if base in _VIEWS or not torch.is_tensor(out):
            return out
        src = next((a for a in args if torch.is_tensor(a)), None)
        if not out.is_cuda and src is not None and src.is_cuda:
            self.d2h += 1
        elif base == "copy_" and len(args) > 1 and torch.is_tensor(args[1]) and args[1].is_cuda and not args[0].is_cuda:
            self.d2h += 1
        elif out.is_cuda:
            self.aten += 1
        return out


def count_tail(fn):
    """-> (ATen GPU ops, C-ABI launches, device-to-host copies) of one call of fn"""
    from pointnet2 import _ext
    real, native = _ext._run, [0]

    def counting(f, anchor, *args):
        native[0] += 1
        return real(f, anchor, *args)

    _ext._run = counting
    try:
        with Count() as c:
            fn()
    finally:
        _ext._run = real
    torch.cuda.synchronize()
    return c.aten, native[0], c.d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inference_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference: needs a GPU (nothing is timed without one)")
    import ap_helper_pq
    import inference
    import synth
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = bench.build_model(0).to(dev).eval()
    cfg = {"remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
           "per_class_proposal": True, "conf_thresh": 0.0, "dataset_config": DatasetConfig()}     # the reference's eval.py
    lines = [f"# python tools/bench_inference.py --points {args.points} --batches {' '.join(map(str, args.batches))} "
             f"--rounds {args.rounds} --iters {args.iters}        ({torch.cuda.get_device_name(0)}, one process)",
             "# eval / bf16, one batch from the forward to its host lists (objects and quads of `last_`); ms per batch: median "
             "over the rounds (spread = max - min); the three routes alternate inside every round"]
    for B in args.batches:
        pool = [synth.make_clouds(100 + i, B, args.points, kind="room").to(dev) for i in range(3)]

        def forward(pc):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                ep = net({"point_clouds": pc})
            ep["point_clouds"] = pc
            return ep

        def parent(i):
            ep = forward(pool[i % 3])
            return ap_helper_pq.parse_predictions(ep, cfg, "last_"), ap_helper_pq.parse_quad_predictions(ep, cfg, "last_")

        eager = inference.CapturedInference(net, pool[0], cfg, graph=False)
        replay = inference.CapturedInference(net, pool[0], cfg)
        assert replay.launch == "hipGraph replay"

        def through(runner):
            def one(i):
                boxes, quads = runner.run(pool[i % 3], next_inputs=pool[(i + 1) % 3])["last_"]
                return boxes.to_lists(), quads.to_lists()
            return one

        routes = {"parent": parent, "eager+L1": through(eager), "replay": through(replay)}
        # the three deliver the same lists on the batch that is timed
        want = parent(0)
        for name in ("eager+L1", "replay"):
            replay.forget_next()
            got = routes[name](0)
            for w, g in zip(want, got):
                assert np.array_equal(w[1], g[1]) and [len(x) for x in w[0]] == [len(x) for x in g[0]], name
        # what follows the forward, counted once per route
        ep = forward(pool[0])
        recs = eager.records["last_"]
        tail_a = count_tail(lambda: (ap_helper_pq.parse_predictions(ep, cfg, "last_"),
                                     ap_helper_pq.parse_quad_predictions(ep, cfg, "last_")))
        tail_b = count_tail(lambda: (ap_helper_pq.detect_predictions(ep, cfg, "last_", out=recs[0]).to_host().to_lists(),
                                     ap_helper_pq.detect_quad_predictions(ep, cfg, "last_", out=recs[1]).to_host().to_lists()))
        for name, (aten, native, d2h) in (("parent", tail_a), ("eager+L1", tail_b)):
            lines.append(f"# batch {B} after the forward, {name:8s}: {aten:3d} ATen GPU ops + {native} C-ABI launches, "
                         f"{d2h} device-to-host copies")
        t = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                eager.forget_next()                          # the route before ran forwards of the same network
                replay.forget_next()
                for i in range(3):
                    fn(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    fn(i)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / args.iters * 1e3)
        med = {n: statistics.median(v) for n, v in t.items()}
        spr = {n: max(v) - min(v) for n, v in t.items()}
        for name in routes:
            verdict = ""
            if name != "parent":
                faster = med[name] < med["parent"] - (spr[name] + spr["parent"])
                verdict = f"   parent / this {med['parent'] / med[name]:5.2f}   " + \
                    ("faster than the parent" if faster else "not faster beyond the spreads")
            lines.append(f"batch {B} {name:9s} {med[name]:8.3f} ms ({spr[name]:.3f})   {B / med[name] * 1e3:8.1f} scenes/s{verdict}")
        del eager, replay
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
