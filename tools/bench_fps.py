#!/usr/bin/env python
"""Furthest-point sampling at the benchmark's sa1 shape (8 scenes x 40 000 points -> 2048): the default kernel (8 points per
thread) against the small-footprint variant (16 per thread, omnipq_furthest_point_sampling_ex flags), event-timed, us per
round.  (The exact PRUNED variant of round 4 -- slower -- left the product library in round 5; DESIGN.md section 10 records
it.)

    python tools/bench_fps.py [--batch 8] [--points 40000] [--samples 2048] [--reps 5]
        --split K[,K2...]   one call against the same sampling in pieces [0, K), [K, K2), ... (omnipq_furthest_point_sampling_resume)
        --lib PATH          A/B against another build of the library (e.g. the parent commit's): the two are alternated
                            --alternations times in this one process, both through omnipq_furthest_point_sampling_ex
"""
import argparse
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
import torch  # noqa: E402

import pointnet2_utils  # noqa: E402
import synth  # noqa: E402


def timed(fn, reps):
    """-> ms per call of fn() (two untimed calls first)"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kind", default="room")
    ap.add_argument("--split", default=None, help="cut points K[,K2...]: time the sampling in these pieces")
    ap.add_argument("--lib", default=None, help="another libomnipq_pointops.so to alternate with this tree's")
    ap.add_argument("--alternations", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    xyz = synth.make_clouds(100, args.batch, args.points, kind=args.kind)[..., :3].contiguous().to(dev)
    ext = pointnet2_utils._ext
    b, n, m = args.batch, args.points, args.samples
    rounds = max(m - 1, 1)
    res = {}
    for name, small in (("every point, 8 per thread", False), ("every point, 16 per thread", True)):
        out = [None]

        def whole():
            out[0] = ext.furthest_point_sampling(xyz, m, small_footprint=small)
        ms = timed(whole, args.reps)
        res[name] = out[0].clone()
        print(f"{name:28s} {ms:7.3f} ms per call = {ms * 1e3 / rounds:6.3f} us per round")
    names = list(res)
    for nm in names[1:]:
        print(f"indices equal ({names[0]} vs {nm}):", bool(torch.equal(res[names[0]], res[nm])))

    idx = torch.zeros((b, m), device=dev, dtype=torch.int32)
    tmp = torch.empty((b, n), device=dev, dtype=torch.float32)
    if args.split:
        cuts = [0] + sorted({int(k) for k in args.split.split(",") if 0 < int(k) < m}) + [m]
        for name, small in (("8 per thread", False), ("16 per thread", True)):
            def one():
                tmp.fill_(1e10)
                ext.furthest_point_sampling_resume(xyz, idx, tmp, 0, m, small_footprint=small)

            def pieces():
                tmp.fill_(1e10)
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    ext.furthest_point_sampling_resume(xyz, idx, tmp, lo, hi - lo, small_footprint=small)
            ms1 = timed(one, args.reps)
            whole_idx = idx.clone()
            msp = timed(pieces, args.reps)
            print(f"split {name:14s} one call {ms1:7.3f} ms; {len(cuts) - 1} pieces at {cuts[1:-1]} {msp:7.3f} ms "
                  f"(+{(msp - ms1) * 1e3:6.1f} us, {(msp - ms1) * 1e3 / max(len(cuts) - 2, 1):5.1f} us per extra piece); "
                  f"indices equal: {bool(torch.equal(idx, whole_idx))}")
    if args.lib:
        libs = {"this tree": ctypes.CDLL(ext.LIB_PATH), "other": ctypes.CDLL(os.path.abspath(args.lib))}
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        print(f"A/B: this tree = {ext.LIB_PATH}; other = {os.path.abspath(args.lib)}")
        for fname, flags in (("8 per thread", 0), ("16 per thread", 1)):
            got = {}
            for alt in range(args.alternations):
                for who, lib in (list(libs.items()) if alt % 2 == 0 else list(libs.items())[::-1]):   # take turns going first
                    def call():
                        tmp.fill_(1e10)
                        rc = lib.omnipq_furthest_point_sampling_ex(b, n, m, ctypes.c_void_p(xyz.data_ptr()),
                                                                   ctypes.c_void_p(tmp.data_ptr()), ctypes.c_void_p(idx.data_ptr()),
                                                                   ctypes.c_uint(flags), stream)
                        assert rc == 0, rc
                    ms = timed(call, args.reps)
                    got.setdefault(who, []).append(ms * 1e3 / rounds)
                    res[(who, fname)] = idx.clone()
                    print(f"A/B {fname:14s} run {alt} {who:10s} {ms:7.3f} ms per call = {ms * 1e3 / rounds:6.3f} us per round")
            spread = {who: max(v) - min(v) for who, v in got.items()}
            mean = {who: sum(v) / len(v) for who, v in got.items()}
            print(f"A/B {fname:14s} mean us per round: this tree {mean['this tree']:.3f}, other {mean['other']:.3f} "
                  f"(difference {mean['this tree'] - mean['other']:+.3f}; run-to-run spread: this tree {spread['this tree']:.3f}, "
                  f"other {spread['other']:.3f}); indices equal: "
                  f"{bool(torch.equal(res[('this tree', fname)], res[('other', fname)]))}")
    ext.fps_check()


if __name__ == "__main__":
    main()
