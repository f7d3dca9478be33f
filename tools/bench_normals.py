#!/usr/bin/env python
"""What the per-point normal estimation (omni-pq_amd/point_normals.py, csrc/point_normals.hip) costs on the device, per stage
and as a whole, over a sweep of the k-NN grid's cell edge -- and what the same recipe costs on the host of the same box.

    device   omnipq_knn, omnipq_normals_plane_fit, `iters` x omnipq_normals_smooth, omnipq_normals_orient and
             omnipq_estimate_normals (all of them in one call), timed with events on the stream: per case `--warmup` calls, then
             `--repeats` timed calls, median and spread (max - min).  Nothing else may run on the card.
    host     the float64 restatement of the same four stages (tests/normals_reference.py) with scipy.spatial.cKDTree for the
             neighbours, limited to 16 threads; wall time, median of `--host-repeats` runs.

The cell is swept as a multiple of r_k = sqrt(k A / (pi n)), the radius that holds k points on a surface of the bounding box's
area A (pointnet2/_ext.py: default_knn_cell); the best multiple is the library's KNN_CELL_FACTOR.

    python tools/bench_normals.py [--points 50000] [--k 100] [--iters 5] [--scenes 1] [--out profiles/normals_ab.txt]

Prints the table, writes it to --out, and prints one JSON line (last line of the output).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

FACTORS = (0.6, 0.7, 0.8, 0.9, 1.0, 1.15, 1.3, 1.5, 1.75, 2.0, 2.5, 3.0)


def device_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), max(out) - min(out)


def host_recipe(xyz, k, iters, repeats):
    """-> (median seconds of the whole recipe, of the neighbour search alone)"""
    from scipy.spatial import cKDTree
    import normals_reference as R
    whole, search = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        p = xyz.astype(np.float64)
        _, idx = cKDTree(p).query(p, k, workers=16)
        t1 = time.perf_counter()
        idx = idx.astype(np.int32)
        nrm = R.plane_fit(xyz, idx)[0]
        for _ in range(iters):
            nrm = R.smooth_step(nrm, idx)[0]
        R.orient(xyz, nrm, R.view_centre(xyz))
        whole.append(time.perf_counter() - t0)
        search.append(t1 - t0)
    return statistics.median(whole), statistics.median(search)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "normals_ab.txt"))
    args = ap.parse_args()
    torch.set_num_threads(16)
    import point_normals
    import synth
    from pointnet2 import _ext
    lib = _ext._lib0
    B, N, K = args.scenes, args.points, args.k
    xyz = synth.make_clouds(0, B, N)
    x = xyz.cuda().contiguous()
    lo, hi = xyz.amin(dim=(0, 1)).tolist(), xyz.amax(dim=(0, 1)).tolist()
    r_k = _ext.default_knn_cell(lo, hi, N, K) / _ext.KNN_CELL_FACTOR
    centre = point_normals.recipe_view_centre(x)
    idx = torch.empty((B, N, K), dtype=torch.int32, device="cuda")
    a, b2 = (torch.empty((B, N, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    ws = torch.empty(int(lib.omnipq_estimate_normals_workspace_bytes(B, N, K)), dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                 # noqa: E731
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)     # noqa: E731

    def check(rc):
        if rc:
            raise RuntimeError(lib.omnipq_error_string(rc).decode())

    def smooth_all():
        src, dst = a, b2
        for _ in range(args.iters):
            check(lib.omnipq_normals_smooth(B, N, K, P(idx), P(src), P(dst), st()))
            src, dst = dst, src

    lines = [f"per-point normals on the device: {B} x synth.room_scene, n = {N}, k = {K}, {args.iters} smoothing steps; "
             f"{torch.cuda.get_device_name(0)}",
             f"device ms by events, median (spread) of {args.repeats} calls after {args.warmup} warm-up calls; "
             f"r_k = sqrt(k A / (pi n)) = {r_k:.4f} m (bounding box {[round(h - l, 2) for l, h in zip(lo, hi)]})",
             "", f"{'cell / r_k':>10} {'cell m':>8} {'knn ms':>18} {'whole recipe ms':>18}"]
    sweep = {}
    for f in FACTORS:
        cell = f * r_k
        knn = device_ms(lambda: check(lib.omnipq_knn(B, N, N, K, cell, P(x), P(x), P(idx), None, P(ws), st())), args.warmup,
                        args.repeats)
        whole = device_ms(lambda: check(lib.omnipq_estimate_normals(B, N, K, args.iters, cell, P(x), P(centre), P(a), P(ws), st())),
                          args.warmup, args.repeats)
        sweep[f] = {"cell": cell, "knn_ms": knn, "recipe_ms": whole}
        lines.append(f"{f:>10.2f} {cell:>8.4f} {knn[0]:>10.3f} ({knn[1]:.3f}) {whole[0]:>10.3f} ({whole[1]:.3f})")
    best = min(sweep, key=lambda f: sweep[f]["recipe_ms"][0])
    cell = best * r_k
    check(lib.omnipq_knn(B, N, N, K, cell, P(x), P(x), P(idx), None, P(ws), st()))
    stages = {"knn": sweep[best]["knn_ms"],
              "plane_fit": device_ms(lambda: check(lib.omnipq_normals_plane_fit(B, N, K, P(x), P(idx), P(a), None, st())),
                                     args.warmup, args.repeats),
              f"smooth x {args.iters}": device_ms(smooth_all, args.warmup, args.repeats),
              "orient": device_ms(lambda: check(lib.omnipq_normals_orient(B, N, P(x), P(centre), P(a), st())), args.warmup,
                                  args.repeats),
              "whole recipe": sweep[best]["recipe_ms"]}
    lines += ["", f"best cell: {best:.2f} r_k = {cell:.4f} m; stages there:"]
    lines += [f"{name:>16} {ms[0]:>10.3f} ms ({ms[1]:.3f})" for name, ms in stages.items()]
    host = host_recipe(xyz[0].numpy(), K, args.iters, args.host_repeats)
    per_scene = stages["whole recipe"][0] / B
    lines += ["", f"host recipe on the same box (float64 restatement, cKDTree with 16 workers), one scene, wall, median of "
              f"{args.host_repeats}: {host[0] * 1e3:.0f} ms, of which the neighbour search {host[1] * 1e3:.0f} ms",
              f"device, per scene: {per_scene:.3f} ms -> {host[0] * 1e3 / per_scene:.0f} x"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(json.dumps({"points": N, "k": K, "iters": args.iters, "scenes": B, "r_k": r_k, "best_factor": best,
                      "sweep": {str(f): v for f, v in sweep.items()}, "stages": stages, "host_s": host[0],
                      "host_search_s": host[1]}))


if __name__ == "__main__":
    main()
