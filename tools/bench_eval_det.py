#!/usr/bin/env python
"""A/B of the detection metrics: the host route (eval_det.eval_det: box3d_iou in Python per detection and ground-truth box,
once per threshold) against the device route (csrc/eval_iou.hip through eval_det.eval_det_device: one IoU pass for all
thresholds, the greedy match on the host) on procedurally generated accumulations of validation size.

    python tools/bench_eval_det.py [--scans 312] [--host-scans 312] [--rounds 3] [--out profiles/eval_det_ab.txt]

Three accumulations, seeds fixed:
    boxes       312 scans, 18 classes, up to 256 proposals kept per scan, listed once per class (per_class_proposal: the score
                is class probability x objectness), axis-aligned (ScanNet)
    boxes_rot   the same with headings (SUN RGB-D style)
    quads       312 scans, up to 256 proposals, up to 32 ground-truth quads, 0.1 thick, one class (accumulated in an
                APCalculator: QUADAPCalculator.compute_metrics is the same call on the same two lists)
Wall time is taken for the whole `compute_metrics` at the thresholds 0.25 and 0.5: on the host route and on the device route
as one calculator per threshold (the reference's arrangement: two IoU passes), and on the device route through
ap_helper_pq.compute_metrics_at (one pass).  The device pass is split into pack / upload / launch / download / match, each
ending in a synchronise.  The host route is timed once, the device route `--rounds` times after a warm-up (median).
`--host-scans N` runs the A/B on the first N scans only (host time grows linearly with the scans: every scan brings its own
pairs) and reports the device route at the full size besides; the file states which.  Both routes must return equal metrics.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))

NUM_CLASS, MAX_PROPOSALS, MAX_QUADS = 18, 256, 32


def corners(center, size, heading):
    """get_3d_box for n boxes: centre (n, 3) in the upright-camera frame, size (n, 3) = (l, w, h), heading (n,) -> (n, 8, 3)"""
    l, w, h = size[:, 0:1], size[:, 1:2], size[:, 2:3]
    x = np.concatenate([l, l, -l, -l, l, l, -l, -l], 1) / 2
    y = np.concatenate([h, h, h, h, -h, -h, -h, -h], 1) / 2
    z = np.concatenate([w, -w, -w, w, w, -w, -w, w], 1) / 2
    c, s = np.cos(heading)[:, None], np.sin(heading)[:, None]
    return np.stack([c * x + s * z + center[:, 0:1], y + center[:, 1:2], -s * x + c * z + center[:, 2:3]], -1)


def make_boxes(scans, rotated, seed):
    """-> (pred_all, gt_all) as APCalculator accumulates them with per_class_proposal"""
    rs = np.random.RandomState(seed)
    pred_all, gt_all = {}, {}
    for img in range(scans):
        n_gt = rs.randint(3, 41)
        gc = np.stack([rs.rand(n_gt) * 8, rs.rand(n_gt) * 0.5 - 1.0, rs.rand(n_gt) * 8], 1)
        gs = 0.3 + rs.rand(n_gt, 3) * 1.7
        gh = (rs.rand(n_gt) - 0.5) * 2 * np.pi if rotated else np.zeros(n_gt)
        gcls = rs.randint(NUM_CLASS, size=n_gt)
        g8 = corners(gc, gs, gh)
        gt_all[img] = [(int(gcls[j]), g8[j]) for j in range(n_gt)]
        k = rs.randint(MAX_PROPOSALS // 4, MAX_PROPOSALS + 1)              # what NMS and the confidence threshold kept
        src = rs.randint(n_gt, size=k)
        near = rs.rand(k) < 0.6                                             # proposals around an object, the rest anywhere
        pc = np.where(near[:, None], gc[src] + rs.randn(k, 3) * 0.15, np.stack([rs.rand(k) * 8, rs.rand(k) * 0.5 - 1.0, rs.rand(k) * 8], 1))
        ps = np.where(near[:, None], gs[src] * (1 + rs.randn(k, 3) * 0.1), 0.3 + rs.rand(k, 3) * 1.7)
        ph = np.where(near, gh[src] + rs.randn(k) * 0.1, (rs.rand(k) - 0.5) * 2 * np.pi) if rotated else np.zeros(k)
        p8 = corners(pc, np.abs(ps) + 0.05, ph)
        logits = rs.randn(k, NUM_CLASS)
        logits[np.arange(k), gcls[src]] += 3.0 * near
        sem = np.exp(logits - logits.max(1, keepdims=True))
        sem = (sem / sem.sum(1, keepdims=True)).astype(np.float32)
        obj = (0.05 + 0.95 * rs.rand(k)).astype(np.float32)
        pred_all[img] = [(c, p8[j], sem[j, c] * obj[j]) for c in range(NUM_CLASS) for j in range(k)]
    return pred_all, gt_all


def make_quads(scans, seed):
    """-> (pred_all, gt_all) as QUADAPCalculator accumulates them: thin oriented boxes of class 1"""
    rs = np.random.RandomState(seed)
    pred_all, gt_all = {}, {}
    for img in range(scans):
        n_gt = rs.randint(4, MAX_QUADS + 1)
        gc = np.stack([rs.rand(n_gt) * 8, rs.rand(n_gt) * 0.2 - 1.3, rs.rand(n_gt) * 8], 1)
        gs = np.stack([1.0 + rs.rand(n_gt) * 4, np.full(n_gt, 0.1), 2.2 + rs.rand(n_gt) * 0.6], 1)     # width, LENGTH, height
        gh = rs.randint(4, size=n_gt) * (np.pi / 2) + rs.randn(n_gt) * 0.05
        g8 = corners(gc, gs, gh)
        gt_all[img] = [(1, g8[j]) for j in range(n_gt)]
        k = rs.randint(MAX_PROPOSALS // 4, MAX_PROPOSALS + 1)
        src = rs.randint(n_gt, size=k)
        pc = gc[src] + rs.randn(k, 3) * np.array([0.05, 0.05, 0.05]) + (rs.rand(k, 1) < 0.3) * rs.randn(k, 3)
        ps = gs[src] * np.stack([1 + rs.randn(k) * 0.1, np.ones(k), 1 + rs.randn(k) * 0.05], 1)
        p8 = corners(pc, np.abs(ps), gh[src] + rs.randn(k) * 0.03)
        prob = rs.rand(k).astype(np.float32)
        pred_all[img] = [(1, p8[j], prob[j]) for j in range(k)]
    return pred_all, gt_all


def head(d, n):
    return {k: d[k] for k in list(d)[:n]}


def same_metrics(a, b):
    return list(a) == list(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def calculators(pred_all, gt_all, iou):
    import ap_helper_pq
    out = []
    for thr in (0.25, 0.5):
        calc = ap_helper_pq.APCalculator(thr, None, iou=iou)
        calc.step(list(pred_all.values()), list(gt_all.values()))
        out.append(calc)
    return out


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def device_split(pred_all, gt_all):
    """-> ({phase: seconds}, metrics at both thresholds, the packed arrays) of one device pass, phase by phase"""
    import ap_helper_pq
    import eval_det
    t = {}
    t["pack"], pack = timed(lambda: eval_det.pack_segments(pred_all, gt_all))
    ovmax, jmax = eval_det.best_on_device(pack, times=t)
    t["match"], triples = timed(lambda: [eval_det.eval_from_best(pack, ovmax, jmax, thr) for thr in (0.25, 0.5)])
    return t, [ap_helper_pq._metrics_dict(rec, ap, None) for rec, _, ap in triples], pack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=312)
    ap.add_argument("--host-scans", type=int, default=312)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_det_ab.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_det: needs a GPU (nothing is timed without one)")
    import ap_helper_pq
    import build as omnipq_build
    host_scans = min(args.host_scans, args.scans)
    lines = [f"# python tools/bench_eval_det.py --scans {args.scans} --host-scans {args.host_scans} --rounds {args.rounds}"
             f"        ({torch.cuda.get_device_name(0)}, one process)",
             f"# library sources {omnipq_build.sources_digest()}",
             "# whole compute_metrics at the thresholds 0.25 and 0.5, wall seconds ending in a synchronise; host: timed once; "
             f"device: median of {args.rounds} rounds after a warm-up (spread = max - min)",
             "# host = eval_det.eval_det, one calculator per threshold; device x2 = iou=\"device\", one calculator per threshold "
             "(two IoU passes); device x1 = compute_metrics_at (one IoU pass)"]
    if host_scans < args.scans:
        lines.append(f"# the A/B runs on the first {host_scans} of {args.scans} scans (host time is linear in the scans: every scan "
                     f"brings its own pairs); the device route is also timed at the full size, and `host est.` there is the "
                     f"measured host time x {args.scans}/{host_scans}")
    print("\n".join(lines), flush=True)

    class Said(list):
        def append(self, line):
            print(line, flush=True)
            list.append(self, line)

    lines = Said(lines)
    wins = []
    for name, make in (("boxes", lambda n: make_boxes(n, False, 1)), ("boxes_rot", lambda n: make_boxes(n, True, 2)),
                       ("quads", lambda n: make_quads(n, 3))):
        full = make(args.scans)
        host_s = None
        for scans in sorted({host_scans, args.scans}):
            pred_all, gt_all = head(full[0], scans), head(full[1], scans)
            device_split(pred_all, gt_all)                                                  # warm-up
            x2, x1, split = [], [], []
            for _ in range(args.rounds):
                dt, m2 = timed(lambda: [c.compute_metrics() for c in calculators(pred_all, gt_all, "device")])
                x2.append(dt)
                calc = calculators(pred_all, gt_all, "device")[0]
                dt, m1 = timed(lambda: ap_helper_pq.compute_metrics_at(calc, (0.25, 0.5)))
                x1.append(dt)
                t, ms, pack = device_split(pred_all, gt_all)
                split.append(t)
                assert all(same_metrics(a, b) and same_metrics(a, c) for a, b, c in zip(m2, m1, ms))
            n_pred, n_gt, n_seg = len(pack["pred_seg"]), len(pack["gt8"]), len(pack["seg_start"]) - 1
            pairs = int(np.diff(pack["seg_start"])[pack["pred_seg"]].sum())
            lines.append(f"{name} {scans} scans: {n_pred} detections, {n_gt} ground-truth boxes in {n_seg} segments, "
                         f"{pairs} IoU pairs per pass")
            if scans == host_scans:
                host_s, mh = timed(lambda: [c.compute_metrics() for c in calculators(pred_all, gt_all, "host")])
                equal = all(same_metrics(a, b) for a, b in zip(mh, m1))
                lines.append(f"{name} {scans} scans: host {host_s:9.3f} s   metrics equal to the device route's: {'yes' if equal else 'NO'}"
                             f"   mAP@0.25 {float(mh[0]['mAP']):.4f} mAP@0.5 {float(mh[1]['mAP']):.4f}")
                assert equal
                wins.append(host_s > max(x2))
                ref = f"host / device x2 {host_s / statistics.median(x2):7.1f}   host / device x1 {host_s / statistics.median(x1):7.1f}"
            else:
                est = host_s * scans / host_scans
                ref = (f"host est. {est:9.3f} s   host est. / device x2 {est / statistics.median(x2):7.1f}   "
                       f"host est. / device x1 {est / statistics.median(x1):7.1f}")
            lines.append(f"{name} {scans} scans: device x2 {statistics.median(x2):7.3f} s ({max(x2) - min(x2):.3f})   "
                         f"device x1 {statistics.median(x1):7.3f} s ({max(x1) - min(x1):.3f})   {ref}")
            med = {k: statistics.median(s[k] for s in split) for k in ("pack", "upload", "launch", "download", "match")}
            lines.append(f"{name} {scans} scans: one device pass: " + "  ".join(f"{k} {v * 1e3:8.2f} ms" for k, v in med.items()))
    lines.append("verdict: " + ("the device route wins on every accumulation (beyond the spread)" if all(wins)
                                else "the device route does NOT win on every accumulation"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
