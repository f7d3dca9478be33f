"""GPU: the ways of running the attention backward (csrc/attention.hip) give the same bits.

The dK/dV program forms delta = sum_d dO*O for itself instead of reading what the dQ program wrote, so the two no longer
depend on each other.  Through the C ABI, on buffers laid out by the helpers of test_gpu_attention_f64.py (NaN-filled,
with guard bands), three ways of computing one backward must agree bit for bit in dQ, dK, dV and delta:
    omnipq_attn_bwd in mode 0   two dependent launches, dK/dV reading the stored delta (the kernels as they were)
    omnipq_attn_bwd in mode 1   one launch with both programs
    omnipq_attn_bwd_dkdv FIRST, then omnipq_attn_bwd_dq, on one stream (dK/dV cannot have read a delta: none was written)
and through autograd, PackedAttention with its dK/dV launch on the key side's stream must return what it returns without,
eagerly and replayed from a captured graph.  What the values ARE is test_gpu_attention_f64.py's business; mode 1 is the
default there.
"""
import ctypes

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import attention_reference as ar
import test_gpu_attention_f64 as f64

pytestmark = pytest.mark.gpu
DEV = f64.DEV
BF16 = torch.bfloat16

# (N, H, L, S, D, p, layout): partial query blocks, partial key blocks, a partial 128-key workgroup, more than one dK/dV
# block, the padded head dimensions, dropout on and off, (N * H) % 8 == 0 (the XCD mapping of att_block) and != 0
CASES = [(2, 8, 40, 72, 36, 0.1, "cross"), (1, 2, 33, 130, 36, 0.5, "cross"), (2, 4, 64, 64, 36, 0.0, "self"),
         (1, 8, 96, 160, 48, 0.1, "cross"), (3, 1, 32, 257, 4, 0.0, "cross"), (1, 8, 1, 1, 36, 0.1, "cross")]


@pytest.fixture(autouse=True)
def _merged_launch_afterwards():
    yield
    import sa_fused
    for lib in sa_fused._ext._LIBS.values():
        lib.omnipq_attn_bwd_mode(1)


@pytest.fixture()
def side_route(monkeypatch):
    """the switch the product ships turned off: a kv_stream is honoured only while it is on"""
    from utils import fused_attention
    monkeypatch.setattr(fused_attention, "CROSS_DKDV_SIDE", True)
    return fused_attention


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("N,H,L,S,D,p,lay", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}x{c[3]}-d{c[4]}-p{c[5]}-{c[6]}" for c in CASES])
def test_three_ways_one_result(N, H, L, S, D, p, lay):
    lib, ext = f64.lib_of(BF16)
    case = dict(L=L, S=S, N=N, H=H, D=D, p=p, layout=lay, dtype=BF16)
    B = N * H
    q, k, v, do = ar.make_inputs(L, S, N, H, D, "randn", 7 * L + S)
    sl = f64.layout(case)
    for name, x in (("q", q), ("k", k), ("v", v), ("do", do)):
        sl[name].put(x, N, H)
    strides = f64.ll(*(x for n in ("q", "k", "v", "o") for x in (sl[n].tok, sl[n].bat)))
    gst = [x for n in ("dq", "dk", "dv") for x in (sl[n].tok, sl[n].bat)]
    seed = torch.tensor([f64.SEED], dtype=torch.int64, device=DEV) if p > 0 else None
    seed_p = ctypes.c_void_p(seed.data_ptr() if seed is not None else 0)
    stream = ext._stream(0)
    lse_buf, lse_p = f64.f32_out(B, L)
    ptr = {n: s.ptr() for n, s in sl.items()}
    assert lib.omnipq_attn_fwd(N, H, L, S, D, ptr["q"], ptr["k"], ptr["v"], ptr["o"], strides, lse_p, p, seed_p, f64.SALT,
                               stream) == 0
    torch.cuda.synchronize()
    inputs = [sl[n].buf for n in ("q", "k", "v", "o", "do")] + [lse_buf]
    before = [b.clone() for b in inputs]
    head = (N, H, L, S, D, ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["do"], strides, lse_p)
    tail = (p, seed_p, f64.SALT, stream)

    def whole(mode):
        def run(delta_p):
            lib.omnipq_attn_bwd_mode(mode)
            assert lib.omnipq_attn_bwd(*head, delta_p, ptr["dq"], ptr["dk"], ptr["dv"], f64.ll(*gst), *tail) == 0
        return run

    def halves(delta_p):
        # dK/dV first: the delta buffer still holds NaN when it runs
        assert lib.omnipq_attn_bwd_dkdv(*head, ptr["dk"], ptr["dv"], f64.ll(*gst[2:]), *tail) == 0
        assert lib.omnipq_attn_bwd_dq(*head, delta_p, ptr["dq"], f64.ll(*gst[:2]), *tail) == 0

    results = []
    for way in (whole(0), whole(1), halves):
        for n in ("dq", "dk", "dv"):
            sl[n].buf.view(torch.int16).fill_(f64.NAN16[BF16])
        delta_buf, delta_p = f64.f32_out(B, L)
        way(delta_p)
        torch.cuda.synchronize()
        got = dict(delta=f64.f32_get(delta_buf, B, L))              # asserts delta's guard bands
        for n in ("dq", "dk", "dv"):
            got[n] = bits(sl[n].view()).cpu()
            assert bool(torch.isfinite(sl[n].view().float()).all()), n
        assert bool(torch.isfinite(got["delta"]).all())
        assert f64.untouched(list(sl.values())), "backward wrote between the rows or into a guard band"
        for b, was in zip(inputs, before):
            assert torch.equal(b.view(torch.int16), was.view(torch.int16)), "backward changed an input"
        results.append(got)
    for other, name in ((results[1], "one launch"), (results[2], "dK/dV before dQ")):
        for n in ("dq", "dk", "dv", "delta"):
            assert torch.equal(results[0][n], other[n]), (name, n)
    assert float(results[0]["dk"].float().abs().max()) > 0


# ---- the autograd route: PackedAttention with its dK/dV launch on the stream of the key side ----------------------

_SIDE = []


def side_stream():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(DEV))
    return _SIDE[0]


def cross_tensors(N, H, L, S, D):
    E = H * D
    gen = torch.Generator().manual_seed(3 * L + S)
    a = (1.5 * torch.randn((N * L, E), generator=gen)).to(BF16).to(DEV).requires_grad_(True)
    kv = torch.cat([1.5 * torch.randn((N * S, E), generator=gen), torch.randn((N * S, E), generator=gen)], dim=1)
    kv = kv.to(BF16).to(DEV).requires_grad_(True)
    g = torch.randn((N * L, E), generator=gen).to(BF16).to(DEV)
    return a, kv, g


def cross_step(a, kv, g, dims, p, use_side):
    """forward and backward of one cross attention whose packed k|v is produced on a side stream, as
    decoder_rows.precompute_key_sides does -> (out, d a, d kv)"""
    from utils import fused_attention
    N, H, L, S = dims
    cur, side = torch.cuda.current_stream(), side_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        b = kv.clone()
    b.record_stream(cur)
    cur.wait_stream(side)
    out = fused_attention.PackedAttention.apply(a, b, L, S, N, H, p, side if use_side else None)
    da, dkv = torch.autograd.grad(out, [a, kv], g)
    cur.wait_stream(side)                    # the test reads d kv on the current stream
    return out, da, dkv


def test_side_stream_dkdv_is_bit_equal_to_the_single_launch(side_route):
    fused_attention = side_route
    N, H, L, S, D, p = 2, 8, 40, 72, 36, 0.1
    a, kv, g = cross_tensors(N, H, L, S, D)
    assert fused_attention.packed_usable(a, kv, H)
    got = []
    try:
        for use_side in (True, False):
            fused_attention.STATE.set_state(DEV, 424242)
            fused_attention.STATE.advance(DEV)                 # the same seed, the salt counter at zero
            got.append([bits(t).cpu() for t in cross_step(a, kv, g, (N, H, L, S), p, use_side)])
    finally:
        fused_attention.STATE.reset()
    for x, y, name in zip(got[0], got[1], ("out", "da", "dkv")):
        assert torch.equal(x, y), name
    assert all(float(x.view(BF16).float().abs().max()) > 0 for x in got[0])
    assert all(bool(torch.isfinite(x.view(BF16).float()).all()) for x in got[0])


def test_side_stream_dkdv_replays_from_a_captured_graph(side_route):
    """forward, backward and the side stream captured once; every replay advances the seed and must equal the eager
    step (without the side launch) for that seed"""
    fused_attention = side_route
    N, H, L, S, D, p = 1, 8, 96, 160, 36, 0.1
    a, kv, g = cross_tensors(N, H, L, S, D)
    state = fused_attention.STATE

    def step(use_side):
        state.advance(DEV)
        return cross_step(a, kv, g, (N, H, L, S), p, use_side)

    try:
        state.set_state(DEV, 1000)
        warm = torch.cuda.Stream(DEV)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            step(True)
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        state.set_state(DEV, 1000)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = step(True)
        replayed = []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            replayed.append([bits(t).cpu() for t in static])
        state.set_state(DEV, 1000)
        eager = [[bits(t).cpu() for t in step(False)] for _ in range(2)]
    finally:
        state.reset()
    for i in range(2):
        for x, y, name in zip(replayed[i], eager[i], ("out", "da", "dkv")):
            assert torch.equal(x, y), (i, name)
    assert not torch.equal(replayed[0][0], replayed[1][0]), "the second replay drew the first one's masks"
    assert all(bool(torch.isfinite(x.view(BF16).float()).all()) for r in replayed for x in r)
