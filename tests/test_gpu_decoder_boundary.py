"""GPU: the entry points that fold the decoder's stage-boundary launches into their neighbours, each held BIT FOR BIT to
the launches it replaces, in both element-type libraries:

  omnipq_add_dropout_layernorm_split                    = omnipq_add_dropout_layernorm, then omnipq_split_rows(out16)
  omnipq_add_dropout_layernorm_bwd_split / _partials_   = omnipq_merge_rows, then the plain backward on the merged gradient
  omnipq_decode_pair_pos16                              = omnipq_decode_pair, then omnipq_pad_rows_e16(pos)
  omnipq_merge_rows_f32 / omnipq_split_rows_sum         = torch.cat + cast / e16(g32 + float(g16)) split in two

Every buffer a kernel writes lies between two guard bands (test_gpu_decoder_f64.Buf).  The shapes are the smallest at which
the index arithmetic differs: two and three scenes, an empty object block, an empty quad block, C = 40 (one partly filled
chunk row per lane) and C = 288 (two chunks per lane), R below and above one workgroup's four rows.
"""
import ctypes

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import decoder_reference as dr
from test_gpu_decoder_f64 import Buf, P, IN, LIBS, LIB_IDS, lib_of, same_bits, seed_buf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = 10001
SHAPES = [(2, 6, 2, 40), (3, 5, 0, 32), (3, 5, 5, 32), (2, 64, 32, 288)]            # (B, p, p0, C)
SHAPE_IDS = ["2x6-2-c40", "3x5-0-c32", "3x5-5-c32", "2x64-32-c288"]


def ln_inputs(B, p, p0, C, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    R = B * p

    def rnd(*shape, dt=torch.float32, scale=1.0):
        return (torch.randn(shape, generator=gen) * scale).to(dt)

    return dict(x=rnd(R, C), y=rnd(R, C, dt=dtype), gamma=1.0 + rnd(C, scale=0.2), beta=rnd(C, scale=0.2),
                pe=rnd(R, C, dt=dtype), g32=rnd(R, C), g16=rnd(R, C, dt=dtype), gpe=rnd(R, C, dt=dtype),
                g_obj=rnd(B * p0, C, dt=dtype), g_quad=rnd(B * (p - p0), C, dt=dtype))


def drop_args(p_drop):
    seed = seed_buf() if p_drop > 0 else None
    return seed, ctypes.c_void_p(seed.data_ptr() if seed is not None else 0)


def ln_forward(lib, stream, inp, R, C, dtype, p_drop, seed_p, with_pe, split=None):
    b = {n: IN(inp[n]) for n in ("x", "y", "gamma", "beta")}
    pe = IN(inp["pe"]) if with_pe else None
    out = dict(out32=Buf(R * C, torch.float32), out16=Buf(R * C, dtype), out_pe=Buf(R * C, dtype) if with_pe else None,
               mean=Buf(R, torch.float32), rstd=Buf(R, torch.float32))
    head = (P(b["x"]), P(b["y"]), P(b["gamma"]), P(b["beta"]), dr.EPS, p_drop, seed_p, dr.SALT, P(out["out32"]),
            P(out["out16"]), P(pe), P(out["out_pe"]), P(out["mean"]), P(out["rstd"]))
    if split is None:
        rc = lib.omnipq_add_dropout_layernorm(R, C, *head, stream)
    else:
        p, p0 = split
        n_obj, n_quad = R // p * p0, R // p * (p - p0)
        out["obj"] = Buf(n_obj * C, dtype) if n_obj else None                # an empty block takes NULL
        out["quad"] = Buf(n_quad * C, dtype) if n_quad else None
        rc = lib.omnipq_add_dropout_layernorm_split(R, C, *head, p, p0, P(out["obj"]), P(out["quad"]), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(v.guards_intact() for v in list(b.values()) + [pe] if v is not None)
    return out


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("with_pe", [False, True], ids=["nope", "pe"])
@pytest.mark.parametrize("p_drop", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_layernorm_split_forward(shape, p_drop, with_pe, dtype):
    lib, stream = lib_of(dtype)
    B, p, p0, C = shape
    R = B * p
    inp = ln_inputs(B, p, p0, C, dtype, 100 + SHAPES.index(shape))
    seed, seed_p = drop_args(p_drop)
    plain = ln_forward(lib, stream, inp, R, C, dtype, p_drop, seed_p, with_pe)
    split = ln_forward(lib, stream, inp, R, C, dtype, p_drop, seed_p, with_pe, (p, p0))
    for name, shp in (("out32", (R, C)), ("out16", (R, C)), ("out_pe", (R, C)), ("mean", (R,)), ("rstd", (R,))):
        if plain[name] is not None:
            assert same_bits(split[name].get(*shp), plain[name].get(*shp)), name
    # ... and the heads' blocks are what omnipq_split_rows copies out of out16
    ob = Buf(B * p0 * C, dtype) if p0 > 0 else None
    qb = Buf(B * (p - p0) * C, dtype) if p0 < p else None
    rc = lib.omnipq_split_rows(B, p, p0, C, P(plain["out16"]), P(ob), P(qb), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want_o, want_q = dr.split_reference(plain["out16"].get(B, p, C), p0)
    if ob is not None:
        assert same_bits(ob.get(B, p0, C), want_o) and same_bits(split["obj"].get(B, p0, C), ob.get(B, p0, C))
    if qb is not None:
        assert same_bits(qb.get(B, p - p0, C), want_q) and same_bits(split["quad"].get(B, p - p0, C), qb.get(B, p - p0, C))
    assert bool(torch.isfinite(split["out32"].get(R, C)).all())


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_layernorm_split_refuses_partial_scenes_and_odd_widths(dtype):
    lib, stream = lib_of(dtype)
    p_ = ctypes.c_void_p(0x1000)                       # never dereferenced: validation comes first
    null = ctypes.c_void_p(0)

    def fwd(R, C, p, p0):
        return lib.omnipq_add_dropout_layernorm_split(R, C, p_, p_, p_, p_, 1e-5, 0.0, null, 0, p_, p_, null, null, p_, p_,
                                                      p, p0, p_, p_, stream)

    assert fwd(13, 40, 6, 2) == EINVAL                 # R % p
    assert fwd(12, 36, 6, 2) == EINVAL                 # C % 8 (a width the plain kernel takes)
    assert fwd(12, 40, 6, 7) == EINVAL and fwd(12, 40, 0, 0) == EINVAL and fwd(12, 40, 6, -1) == EINVAL


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("p_drop", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_layernorm_split_backward(shape, p_drop, dtype):
    """All eight presence combinations of g16 / g_obj16 / g_quad16 (times g32 and g16_pe present or absent): dx, dy and the
    per-workgroup partials of the split entry points against omnipq_merge_rows followed by the plain backward; the atomic
    variant's dx and dy the same, its parameter sums (whose order is not fixed) only against the partials' sum."""
    lib, stream = lib_of(dtype)
    B, p, p0, C = shape
    R = B * p
    inp = ln_inputs(B, p, p0, C, dtype, 200 + SHAPES.index(shape))
    seed, seed_p = drop_args(p_drop)
    fw = ln_forward(lib, stream, inp, R, C, dtype, p_drop, seed_p, False)
    b = {n: IN(inp[n]) for n in ("x", "y", "gamma", "g32", "g16", "gpe")}
    b["g_obj"] = IN(inp["g_obj"]) if p0 > 0 else None
    b["g_quad"] = IN(inp["g_quad"]) if p0 < p else None
    blocks = int(lib.omnipq_add_dropout_layernorm_bwd_blocks(R))
    fixed = (P(b["x"]), P(b["y"]), P(b["gamma"]), p_drop, seed_p, dr.SALT, P(fw["mean"]), P(fw["rstd"]))
    combos = 0
    for mask in range(32):
        has16, has_obj, has_quad, has32, has_pe = (bool(mask >> k & 1) for k in range(5))
        g16, g_obj, g_quad = b["g16"] if has16 else None, b["g_obj"] if has_obj else None, b["g_quad"] if has_quad else None
        g32, gpe = b["g32"] if has32 else None, b["gpe"] if has_pe else None
        # the two launches this replaces
        merged = Buf(R * C, dtype)
        rc = lib.omnipq_merge_rows(B, p, p0, C, P(g_obj), P(g_quad), P(g16), P(merged), stream)
        assert rc == 0, rc
        want = dict(dx=Buf(R * C, torch.float32), dy=Buf(R * C, dtype), part=Buf(blocks * 2 * C, torch.float32))
        rc = lib.omnipq_add_dropout_layernorm_bwd_partials(R, C, *fixed, P(g32), P(merged), P(gpe), P(want["dx"]),
                                                           P(want["dy"]), P(want["part"]), stream)
        assert rc == 0, rc
        got = dict(dx=Buf(R * C, torch.float32), dy=Buf(R * C, dtype), part=Buf(blocks * 2 * C, torch.float32))
        rc = lib.omnipq_add_dropout_layernorm_bwd_partials_split(R, C, *fixed, P(g32), P(g16), P(gpe), P(got["dx"]),
                                                                 P(got["dy"]), P(got["part"]), p, p0, P(g_obj), P(g_quad),
                                                                 stream)
        assert rc == 0, rc
        atom = dict(dx=Buf(R * C, torch.float32), dy=Buf(R * C, dtype),
                    dgb=Buf(2 * C, torch.float32, torch.zeros(2 * C)))
        rc = lib.omnipq_add_dropout_layernorm_bwd_split(R, C, *fixed, P(g32), P(g16), P(gpe), P(atom["dx"]), P(atom["dy"]),
                                                        P(atom["dgb"]), p, p0, P(g_obj), P(g_quad), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for name, shp in (("dx", (R, C)), ("dy", (R, C)), ("part", (blocks, 2 * C))):
            assert same_bits(got[name].get(*shp), want[name].get(*shp)), (mask, name)
        assert same_bits(atom["dx"].get(R, C), want["dx"].get(R, C)), mask
        assert same_bits(atom["dy"].get(R, C), want["dy"].get(R, C)), mask
        total = want["part"].get(blocks, 2 * C).double().sum(0)
        mag = want["part"].get(blocks, 2 * C).double().abs().sum(0)
        # f32 sums of `blocks` partials in two orders: each within blocks * 2^-24 of the exact sum of magnitudes
        assert bool(((atom["dgb"].get(2 * C).double() - total).abs() <= (blocks + 1) * 2.0 ** -23 * mag + 1e-30).all()), mask
        combos += 1
    assert combos == 32
    assert all(v is None or v.guards_intact() for v in b.values())
    assert bool(torch.isfinite(want["dx"].get(R, C)).all())


# ---- omnipq_decode_pair_pos16 ----------------------------------------------------------------------------------------------

NH, NS, NCLS = 3, 5, 7


def decode_pair(lib, stream, B, K, Kq, dtype, inp, kpad):
    yh, yq, bh, bq, means = (IN(inp[n]) for n in ("yh", "yq", "bh", "bq", "means"))
    Rh, Rq = B * K, B * Kq
    f32 = torch.float32
    outs_h = [Buf(Rh * 2, dtype), Buf(Rh * 3, f32), Buf(Rh * NH, dtype), Buf(Rh * NH, dtype), Buf(Rh * NH, dtype),
              Buf(Rh * NS, dtype), Buf(Rh * NS * 3, dtype), Buf(Rh * NS * 3, f32), Buf(Rh * 3, f32), Buf(Rh * NCLS, dtype)]
    outs_q = [Buf(Rq * 2, dtype), Buf(Rq * 3, f32), Buf(Rq * 3, dtype), Buf(Rq * 2, dtype)]
    norm, pos = Buf(1, f32), Buf(B * (K + Kq) * 3, f32)
    ph = (ctypes.c_void_p * 10)(*[o.ptr().value for o in outs_h])
    pq = (ctypes.c_void_p * 4)(*[o.ptr().value for o in outs_q])
    args = (Rh, K, NH, NS, NCLS, P(yh), inp["yh"].shape[1], P(bh), P(means), 3.14159 / NH, ph, Rq, Kq, P(yq),
            inp["yq"].shape[1], P(bq), pq, P(norm), P(pos))
    pos16 = None
    if kpad is None:
        rc = lib.omnipq_decode_pair(*args, stream)
    else:
        pos16 = Buf(B * (K + Kq) * kpad, dtype)
        rc = lib.omnipq_decode_pair_pos16(*args, P(pos16), kpad, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(v.guards_intact() for v in (yh, yq, bh, bq, means))
    return outs_h + outs_q + [norm, pos], pos16


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("kpad", [32, 8, 3])
@pytest.mark.parametrize("K,Kq", [(3, 2), (256, 256)])
def test_decode_pair_pos16(K, Kq, kpad, dtype):
    lib, stream = lib_of(dtype)
    B = 2
    gen = torch.Generator().manual_seed(300 + K)
    ldh = (5 + 2 * NH + 4 * NS + NCLS + 7) // 8 * 8
    inp = dict(yh=torch.randn((B * K, ldh), generator=gen).to(dtype), yq=torch.randn((B * Kq, 16), generator=gen).to(dtype),
               bh=torch.randn((B * K, 3), generator=gen) * 3, bq=torch.randn((B * Kq, 3), generator=gen) * 3,
               means=torch.rand((NS, 3), generator=gen) + 0.5)
    want, _ = decode_pair(lib, stream, B, K, Kq, dtype, inp, None)
    got, pos16 = decode_pair(lib, stream, B, K, Kq, dtype, inp, kpad)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g.get(g.n), w.get(w.n)), i
    n = B * (K + Kq)
    ref16 = Buf(n * kpad, dtype)
    rc = lib.omnipq_pad_rows_e16(n, 3, kpad, 3, P(want[-1]), 1, P(ref16), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert same_bits(pos16.get(n, kpad), ref16.get(n, kpad))
    rows = pos16.get(n, kpad)
    assert same_bits(rows[:, :3], want[-1].get(n, 3).to(dtype))                       # one rounding of the stored f32 value
    assert bool((rows[:, 3:].view(torch.int16) == 0).all())                            # exact (+0) zeros behind it


# ---- the decoder's entry: join, and its gradient -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_join_rows_and_its_gradient(shape, dtype):
    lib, stream = lib_of(dtype)
    B, p, p0, C = shape
    gen = torch.Generator().manual_seed(400 + SHAPES.index(shape))
    obj = torch.randn((B, p0, C), generator=gen).to(dtype)
    quad = torch.randn((B, p - p0, C), generator=gen).to(dtype)
    ob, qb = IN(obj) if p0 > 0 else None, IN(quad) if p0 < p else None
    out32, out16 = Buf(B * p * C, torch.float32), Buf(B * p * C, dtype)
    rc = lib.omnipq_merge_rows_f32(B, p, p0, C, P(ob), P(qb), P(out32), P(out16), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    joint = torch.cat([obj, quad], 1)
    assert same_bits(out16.get(B, p, C), joint) and same_bits(out32.get(B, p, C), joint.float())
    assert all(v is None or v.guards_intact() for v in (ob, qb))
    g32 = torch.randn((B, p, C), generator=gen)
    g16 = torch.randn((B, p, C), generator=gen).to(dtype)
    g16.view(torch.int16)[0, 0, 0] = -32768                                  # a -0 that must survive when g32 is absent
    for a, h in ((g32, g16), (g32, None), (None, g16)):
        ab, hb = IN(a), IN(h)
        d_obj = Buf(B * p0 * C, dtype) if p0 > 0 else None
        d_quad = Buf(B * (p - p0) * C, dtype) if p0 < p else None
        rc = lib.omnipq_split_rows_sum(B, p, p0, C, P(ab), P(hb), P(d_obj), P(d_quad), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        want = h if a is None else a.to(dtype) if h is None else (a + h.float()).to(dtype)
        want_o, want_q = dr.split_reference(want, p0)
        if d_obj is not None:
            assert same_bits(d_obj.get(B, p0, C), want_o), (a is None, h is None)
        if d_quad is not None:
            assert same_bits(d_quad.get(B, p - p0, C), want_q), (a is None, h is None)
