#!/usr/bin/env python
"""Attention kernels alone (csrc/attention.hip) over key counts: where a launch's time goes -- the part that does not
depend on the number of keys (prologue, merge, store) against the part per 128 keys (one iteration of the four waves).

    python tools/bench_attn.py [--dropout 0.1] [--reps 200]
    python tools/bench_attn.py --step-shapes [--bwd-mode 0|1]      the backward alone at the decoder's two shapes, packed layout
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models", "omni-pq_amd/models/utils"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--keys", type=int, nargs="*", default=[32, 128, 256, 512, 1024, 2048])
    ap.add_argument("--bwd-mode", type=int, default=None, choices=[0, 1],
                    help="omnipq_attn_bwd_mode: 0 = dQ then dK/dV as two dependent launches, 1 = one launch (the default)")
    ap.add_argument("--step-shapes", action="store_true",
                    help="time PackedAttention's backward at the captured step's shapes: self 512 x 512, cross 512 x 1024")
    args = ap.parse_args()
    import fused_attention as fa
    dev = torch.device("cuda", 0)
    if args.bwd_mode is not None:
        for lib in fa.sa_fused._ext._LIBS.values():
            lib.omnipq_attn_bwd_mode(args.bwd_mode)
    if args.step_shapes:
        return step_shapes(fa, dev, args)
    N, H, E, L = 8, 8, 288, 256
    torch.manual_seed(0)
    print(f"L={L} N={N} H={H} E={E} dropout={args.dropout}   us per launch (graph of {args.reps} launches)")
    for S in args.keys:
        q = torch.randn(L, N, E, device=dev).to(fa.E16.dtype).requires_grad_(True)
        k = torch.randn(S, N, E, device=dev).to(fa.E16.dtype).requires_grad_(True)
        v = torch.randn(S, N, E, device=dev).to(fa.E16.dtype).requires_grad_(True)
        d_o = torch.randn(L, N, E, device=dev).to(fa.E16.dtype)
        t_f = timed(lambda: fa.FusedAttention.apply(q.detach(), k.detach(), v.detach(), H, args.dropout), args.reps)

        def fb():
            o = fa.FusedAttention.apply(q, k, v, H, args.dropout)
            torch.autograd.grad(o, (q, k, v), d_o)
        t_fb = timed(fb, args.reps)
        print(f"S={S:5d}  fwd {t_f:7.2f}   fwd+bwd {t_fb:7.2f}   bwd {t_fb - t_f:7.2f}")


def step_shapes(fa, dev, args):
    """us per backward of the packed layout (decoder_rows.run): self attention, cross attention as one call, and cross
    attention with dK/dV on a second stream (each graph replay holds --reps backward passes)"""
    N, H, E = 8, 8, 288
    torch.manual_seed(0)
    side = torch.cuda.Stream(dev)
    fa.CROSS_DKDV_SIDE = True             # honour the kv_stream of the third case (the product ships this switch off)
    mode = "default" if args.bwd_mode is None else args.bwd_mode
    print(f"N={N} H={H} E={E} dropout={args.dropout} bwd-mode={mode}   us per backward = (fwd+bwd) - fwd, graphs of {args.reps}")
    for name, L, S, kv_stream in (("self", 512, 512, None), ("cross", 512, 1024, None), ("cross, dK/dV on a side stream", 512, 1024, side)):
        if name == "self":
            a = torch.randn(N * L, 3 * E, device=dev).to(fa.E16.dtype).requires_grad_(True)
            b = None
        else:
            a = torch.randn(N * L, E, device=dev).to(fa.E16.dtype).requires_grad_(True)
            b = torch.randn(N * S, 2 * E, device=dev).to(fa.E16.dtype).requires_grad_(True)
        d_o = torch.randn(N * L, E, device=dev).to(fa.E16.dtype)
        leaves = (a,) if b is None else (a, b)

        # the forward belongs inside the captured function: a node's backward runs on the stream of its forward, and that
        # has to be the capturing stream
        def fwd():
            with torch.no_grad():
                fa.PackedAttention.apply(a, b, L, S, N, H, args.dropout, kv_stream)

        def fwd_bwd():
            o = fa.PackedAttention.apply(a, b, L, S, N, H, args.dropout, kv_stream)
            torch.autograd.grad(o, leaves, d_o)
            if kv_stream is not None:
                torch.cuda.current_stream().wait_stream(kv_stream)
        t_f = sorted(timed(fwd, args.reps) for _ in range(5))[2]
        runs = sorted(timed(fwd_bwd, args.reps) - t_f for _ in range(5))
        print(f"{name:32s} L={L} S={S}   fwd {t_f:6.2f}   bwd: median {runs[2]:7.2f}   min {runs[0]:7.2f}   max {runs[4]:7.2f}")


if __name__ == "__main__":
    main()
