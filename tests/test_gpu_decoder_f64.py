"""GPU: the decoder's row kernels (csrc/decoder_ops.hip) through the C ABI against the float64 reference, ELEMENT BY ELEMENT.

Every entry point of decoder_ops.hip is called directly, in both libraries (bfloat16 and IEEE half), on buffers this module
lays out itself: each buffer, input or output, sits between two guard bands and is filled with a NaN pattern beforehand.
Every element a kernel owns must be finite and inside the bound tests/decoder_reference.py derives from the kernel's
roundings (no exceptions, no norms) -- mean and rstd like any other output -- every guard element must still hold the
pattern, and a kernel that reads past an input poisons its result.  The dropout mask is the restated hash of
decoder_reference.keep_mask, never a probe of the kernel.  The cases are decoder_reference's tables; the CPU suite holds an
emulation of the kernels' arithmetic, and eleven mutants of it, against the same bounds on the same cases
(tests/test_decoder_reference.py).

Each test prints the largest error / bound ratio per output (`RATIO <library> <case>: out32=... out16=...`, pytest -s).
Largest ratios per library and output over all cases, measured on an MI355X (bfloat16 | half, the case that set it):
    LayerNorm   mean    0.126 | 0.118   stride-fwd              rstd    0.243 | 0.243   kind-constant-noy
                out32   0.312 | 0.469   stride-fwd, C-252       out16   0.664 | 0.664   one e16 rounding: 1 / MARGIN
                out_pe  0.664 | 0.665                           dx      0.182 | 0.182   kind-constant-noy
                dy      0.663 | 0.662                           dgb     0.205 | 0.205   R-4
    param_reduce        0.268 | 0.268   the 32 mixed items (0.19 is typical of a single block count)
    relu + dropout      0.644 | 0.657   p = 0.9; exactly 0 at p = 0, 0.5, 1e-12 (the scale is a power of two); same backward
    add_to_e16, merge   0.664 | 0.666   add_n  0.667 | 0.667 (two f32 terms: one rounding, the whole bound / MARGIN)
Nothing is above 1 / MARGIN: the e16 outputs sit at one worst-case store rounding, the f32 outputs at 0.1 - 0.5 of a bound
that counts every rounding on the longest path at its worst.  The emulation's table (tests/test_decoder_reference.py) is
the same to two digits except rstd and dgb (hardware rsqrt, atomics in another order).
"""
import ctypes

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import capi
import decoder_reference as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # elements in front of and behind every buffer (256 / 128 bytes: 16-byte alignment is kept)
PATTERN = {torch.float32: (torch.int32, 0x7FC00001), torch.bfloat16: (torch.int16, 0x7FC1), torch.float16: (torch.int16, 0x7E01)}
LIBS = [torch.bfloat16, torch.float16]
LIB_IDS = ["bf16", "f16"]


def lib_of(dtype):
    lib, ext = capi.lib_of(dtype)
    if lib is None:
        assert dtype is torch.float16 and ext.LIB_F16_PATH is None
        pytest.skip("no IEEE-half library in this build")
    return lib, ext._stream(0)


class Buf:
    """`numel` elements between two guard bands, all of it the NaN pattern of the type; `data` (at most numel elements) is
    copied to the front of the owned part."""

    def __init__(self, numel, dtype, data=None):
        self.n, self.dtype = numel, dtype
        self.it, self.pat = PATTERN[dtype]
        self.t = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
        self.t.view(self.it).fill_(self.pat)
        if data is not None:
            assert data.dtype is dtype and data.numel() <= numel
            self.t[GUARD:GUARD + data.numel()].copy_(data.reshape(-1))

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())

    def bits(self):
        return self.t.view(self.it)

    def guards_intact(self):
        b = self.bits()
        return bool((b[:GUARD] == self.pat).all()) and bool((b[GUARD + self.n:] == self.pat).all())

    def pattern_from(self, k):
        """the owned elements from k on still hold the pattern"""
        return bool((self.bits()[GUARD + k:GUARD + self.n] == self.pat).all())

    def get(self, *shape, numel=None):
        assert self.guards_intact(), "wrote outside the buffer"
        k = self.n if numel is None else numel
        return self.t[GUARD:GUARD + k].cpu().reshape(*shape)


def P(buf):
    return ctypes.c_void_p(0) if buf is None else buf.ptr()


def IN(t):
    return None if t is None else Buf(t.numel(), t.dtype, t)


def seed_buf():
    return torch.tensor([dr.SEED], dtype=torch.int64, device=DEV)


def report(libname, id, rat):
    print(f"\n  RATIO {libname} {id}: {dr.fmt(rat)}")
    assert not dr.outside(rat), (libname, id, dr.outside(rat))


def same_bits(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype is not torch.float32 else a.view(torch.int32),
                       b.view(torch.int16) if b.dtype is not torch.float32 else b.view(torch.int32))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", dr.CASE_IDS)
def test_layernorm_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    case = dr.case_of(id)
    R, C, p, outs, route = (case[n] for n in ("R", "C", "p", "outs", "route"))
    inp = dr.case_inputs(case, dtype)
    keep = dr.case_mask(case)
    drop = case["y"] and p > 0
    seed = seed_buf() if drop else None                                      # p = 0: no seed word is read, NULL is legal
    seed_p = ctypes.c_void_p(seed.data_ptr() if drop else 0)
    b = {n: IN(inp[n]) for n in ("x", "y", "gamma", "beta", "pe", "g32", "g16", "gpe")}
    out32 = Buf(R * C, torch.float32) if outs in ("32", "both", "pe") else None
    out16 = Buf(R * C, dtype) if outs in ("16", "both", "pe") else None
    out_pe = Buf(R * C, dtype) if outs == "pe" else None
    mean, rstd = Buf(R, torch.float32), Buf(R, torch.float32)
    rc = lib.omnipq_add_dropout_layernorm(R, C, P(b["x"]), P(b["y"]), P(b["gamma"]), P(b["beta"]), dr.EPS, p, seed_p, dr.SALT,
                                          P(out32), P(out16), P(b["pe"]), P(out_pe), P(mean), P(rstd), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(mean=mean.get(R), rstd=rstd.get(R))
    for name, buf in (("out32", out32), ("out16", out16), ("out_pe", out_pe)):
        if buf is not None:
            got[name] = buf.get(R, C)
    dx = Buf(R * C, torch.float32)
    dy = Buf(R * C, dtype) if case["y"] else None
    blocks = int(lib.omnipq_add_dropout_layernorm_bwd_blocks(R))
    assert blocks == dr.ln_blocks(R)
    if route == "atomic":
        dgb = Buf(2 * C, torch.float32, inp["acc0"])
        rc = lib.omnipq_add_dropout_layernorm_bwd(R, C, P(b["x"]), P(b["y"]), P(b["gamma"]), p, seed_p, dr.SALT, P(mean), P(rstd),
                                                  P(b["g32"]), P(b["g16"]), P(b["gpe"]), P(dx), P(dy), P(dgb), stream)
    else:
        part = Buf((blocks + 1) * 2 * C, torch.float32)                      # one row more than the kernel may write
        rc = lib.omnipq_add_dropout_layernorm_bwd_partials(R, C, P(b["x"]), P(b["y"]), P(b["gamma"]), p, seed_p, dr.SALT, P(mean),
                                                           P(rstd), P(b["g32"]), P(b["g16"]), P(b["gpe"]), P(dx), P(dy), P(part),
                                                           stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got["dx"] = dx.get(R, C)
    if dy is not None:
        got["dy"] = dy.get(R, C)
    if route == "atomic":
        got["dgb"] = dgb.get(2 * C)
    else:
        rows = part.get(blocks + 1, 2 * C)[:blocks]
        assert bool(torch.isfinite(rows).all()), "a partial row kept the NaN fill"
        assert part.pattern_from(blocks * 2 * C), "wrote past the last partial row"
        got["dgb"] = rows.double().sum(dim=0)
    assert same_bits(mean.get(R), got["mean"]) and same_bits(rstd.get(R), got["rstd"]), "backward changed mean / rstd"
    for name, buf in b.items():
        assert buf is None or (buf.guards_intact() and same_bits(buf.get(buf.n), inp[name].reshape(-1))), name
    ref = dr.reference(inp, keep, p)
    rat = dr.ln_ratios(got, ref, dr.bounds(ref, dtype, route))
    expect = set(dr.LN_OUTPUTS) - (set() if case["y"] else {"dy"}) - {n for n, bf in (("out32", out32), ("out16", out16),
                                                                                    ("out_pe", out_pe)) if bf is None}
    assert set(rat) == expect
    report(LIB_IDS[LIBS.index(dtype)], id, rat)
    if drop:                                                                  # dropped elements of dy are +0, bit for bit
        assert bool((got["dy"].view(torch.int16)[~keep] == 0).all())
        n = keep.numel()
        if n >= 10000:
            assert abs(float(keep.float().mean()) - (1 - p)) < 5.0 * (p * (1 - p) / n) ** 0.5


# ---- omnipq_layernorm_param_reduce ----------------------------------------------------------------------------------------

def run_reduce(lib, stream, items, width):
    """items: [(part (blocks, 2C), out0 (2C))]; every out buffer is `width` wide.  -> [out (2C) on the CPU]"""
    n = len(items)
    parts = [IN(part) for part, _ in items]
    outs = [Buf(width, torch.float32, out0) for _, out0 in items]
    rc = lib.omnipq_layernorm_param_reduce(n, (ctypes.c_void_p * n)(*[x.ptr().value for x in parts]),
                                           (ctypes.c_int * n)(*[part.shape[0] for part, _ in items]),
                                           (ctypes.c_int * n)(*[part.shape[1] // 2 for part, _ in items]),
                                           (ctypes.c_void_p * n)(*[x.ptr().value for x in outs]), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = []
    for (part, out0), pb, ob in zip(items, parts, outs):
        assert pb.guards_intact()
        assert ob.pattern_from(part.shape[1]), "columns >= 2C of an item were written"
        got.append(ob.get(part.shape[1], numel=part.shape[1]))
    return got


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("blocks", dr.REDUCE_BLOCKS)
def test_param_reduce_block_counts(blocks, dtype):
    lib, stream = lib_of(dtype)
    part, out0 = dr.reduce_inputs(blocks, 260, blocks)
    got, = run_reduce(lib, stream, [(part, out0)], 2 * 260 + 64)
    rat = dr.ratios(dict(out=got), dict(out=dr.reduce_reference(part, out0)), dict(out=dr.reduce_bound(part, out0)))
    report(LIB_IDS[LIBS.index(dtype)], f"reduce-{blocks}", rat)


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_param_reduce_mixed_items_in_one_launch(dtype):
    lib, stream = lib_of(dtype)
    items = [dr.reduce_inputs(blocks, C, 100 + i) for i, (blocks, C) in enumerate(dr.reduce_items())]
    got = run_reduce(lib, stream, items, 2 * 1024)
    worst = {}
    for i, ((part, out0), g) in enumerate(zip(items, got)):
        rat = dr.ratios(dict(out=g), dict(out=dr.reduce_reference(part, out0)), dict(out=dr.reduce_bound(part, out0)))
        assert not dr.outside(rat), (i, part.shape, rat)
        worst = rat if not worst or rat["out"][0] > worst["out"][0] else worst
    report(LIB_IDS[LIBS.index(dtype)], "reduce-mixed-32", worst)


# ---- ReLU + dropout and its backward --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("n,p", [(4, 0.5), (4 * 37, 0.0), (4 * 37, 0.1), (4096, 0.5), (4096, 1e-12), (4096, 0.9),
                                 (dr.FLAT_STRIDE + 4, 0.1)])
def test_relu_dropout_and_its_backward(n, p, dtype):
    lib, stream = lib_of(dtype)
    assert n in dr.FLAT_NS or n == 4096
    h = dr.flat_inputs(n, dtype, 1)
    keep = dr.keep_mask(dr.SEED, dr.SALT, p, 1, n).reshape(n)
    seed = seed_buf()
    hb = IN(h)
    rc = lib.omnipq_relu_dropout(n, P(hb), p, ctypes.c_void_p(seed.data_ptr() if p > 0 else 0), dr.SALT, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = hb.get(n)
    ref = dr.relu_dropout_reference(h, keep, p)
    assert torch.equal(out.view(torch.int16) != 0, keep & (h.double() > 0)), "the mask is not the restated one"
    assert same_bits(out, dr.relu_dropout_emulate(h, keep, p))               # kept values are round(h * f32(1 / (1 - p)))
    if p == 0.5:
        assert same_bits(out, torch.where(keep & (h.double() > 0), (2.0 * h.float()).to(dtype), torch.zeros((), dtype=dtype)))
    rat = dr.ratios(dict(h=out), dict(h=ref), dict(h=dr.scaled_bound(ref, dtype)))
    d = dr.flat_inputs(n, dtype, 2).roll(1)
    db, ob = IN(d), Buf(n, dtype)
    rc = lib.omnipq_relu_dropout_bwd(n, P(hb), P(db), P(ob), p, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    dout = ob.get(n)
    assert same_bits(hb.get(n), out) and same_bits(db.get(n), d)
    refb = dr.relu_dropout_bwd_reference(out, d, p)
    gated = ~(out.double() > 0)
    assert bool((dout.view(torch.int16)[gated] == 0).all()), "the gate is not h > 0"
    assert same_bits(dout, dr.relu_dropout_bwd_emulate(out, d, p))
    rat.update(dr.ratios(dict(d=dout), dict(d=refb), dict(d=dr.scaled_bound(refb, dtype))))
    report(LIB_IDS[LIBS.index(dtype)], f"relu-{n}-{p}", rat)
    if n >= 100000 and p > 0:
        assert abs(float(keep.float().mean()) - (1 - p)) < 5.0 * (p * (1 - p) / n) ** 0.5


# ---- add_to_e16 / add_n ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("a_f32", [True, False], ids=["a-f32", "a-e16"])
@pytest.mark.parametrize("n", dr.FLAT_NS)
def test_add_to_e16(n, a_f32, dtype):
    lib, stream = lib_of(dtype)
    a, b = dr.addn_sources(2, n, torch.float32, 7)
    a[-4:] = torch.tensor([-0.0, -0.0, 0.0, 1.0])                          # against b's +-0 and subnormals at n = 4
    a, b = (a if a_f32 else a.to(dtype)), dr.flat_inputs(n, dtype, 3)
    ab, bb, ob = IN(a), IN(b), Buf(n, dtype)
    rc = lib.omnipq_add_to_e16(n, P(ab), int(a_f32), P(bb), P(ob), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = ob.get(n)
    assert ab.guards_intact() and bb.guards_intact()
    tot, bnd = dr.sum_bound([a, b], dtype)
    report(LIB_IDS[LIBS.index(dtype)], f"add_to_e16-{n}-{'f32' if a_f32 else 'e16'}", dr.ratios(dict(s=got), dict(s=tot), dict(s=bnd)))
    assert same_bits(got, (a.float() + b.float()).to(dtype))                 # one f32 addition, one rounding


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("e16", [True, False], ids=["e16", "f32"])
@pytest.mark.parametrize("count", dr.ADDN_COUNTS)
@pytest.mark.parametrize("n", dr.ADDN_NS)
def test_add_n(n, count, e16, dtype):
    lib, stream = lib_of(dtype)
    dt = dtype if e16 else torch.float32
    srcs = dr.addn_sources(count, n, dt, count)
    bufs, ob = [IN(s) for s in srcs], Buf(n, dt)
    rc = lib.omnipq_add_n(count, (ctypes.c_void_p * count)(*[x.ptr().value for x in bufs]), n, int(e16), P(ob), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = ob.get(n)
    assert all(x.guards_intact() for x in bufs)
    tot, bnd = dr.sum_bound(srcs, dt if e16 else None)
    report(LIB_IDS[LIBS.index(dtype)], f"add_n-{n}-{count}-{'e16' if e16 else 'f32'}", dr.ratios(dict(s=got), dict(s=tot), dict(s=bnd)))
    if count == 1:
        assert same_bits(got, dr.add_n_emulate(srcs, dt))                    # 0 + x: x itself, but for -0 -> +0


# ---- pad_rows_e16 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("x_f32", [True, False], ids=["x-f32", "x-e16"])
@pytest.mark.parametrize("i", range(len(dr.PAD_CASES)))
def test_pad_rows_e16(i, x_f32, dtype):
    lib, stream = lib_of(dtype)
    n, cin, k, ldx = (dr.PAD_CASES[i][m] for m in ("n", "cin", "k", "ldx"))
    dt = torch.float32 if x_f32 else dtype
    gen = torch.Generator().manual_seed(6000 + i)
    x = torch.randn((n, ldx), generator=gen).to(dt)
    x[:, cin:] = float("nan")                                                # the pitch's spare columns: never read
    if cin:
        x[0, 0], x[n - 1, cin - 1] = -0.0, 2.0 ** -20
    xb, ob = IN(x), Buf(n * k, dtype)
    rc = lib.omnipq_pad_rows_e16(n, cin, k, ldx, P(xb), int(x_f32), P(ob), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = ob.get(n, k)
    assert bool((got[:, cin:].view(torch.int16) == 0).all()), "padding columns are not +0"
    assert same_bits(got, dr.pad_reference(x, cin, k, dtype))
    assert xb.guards_intact()


# ---- split_rows / merge_rows -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("i", range(len(dr.SPLIT_CASES)))
def test_split_rows_and_merge_rows(i, dtype):
    lib, stream = lib_of(dtype)
    b, p, p0, c = (dr.SPLIT_CASES[i][m] for m in ("b", "p", "p0", "c"))
    gen = torch.Generator().manual_seed(7000 + i)
    x = torch.randn((b, p, c), generator=gen).to(dtype)
    xb = IN(x)
    ob = Buf(b * p0 * c, dtype) if p0 > 0 else None                          # an empty half takes NULL
    qb = Buf(b * (p - p0) * c, dtype) if p0 < p else None
    rc = lib.omnipq_split_rows(b, p, p0, c, P(xb), P(ob), P(qb), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want_o, want_q = dr.split_reference(x, p0)
    if ob is not None:
        assert same_bits(ob.get(b, p0, c), want_o)
    if qb is not None:
        assert same_bits(qb.get(b, p - p0, c), want_q)
    assert xb.guards_intact()
    g_obj = torch.randn((b, p0, c), generator=gen).to(dtype)
    g_quad = torch.randn((b, p - p0, c), generator=gen).to(dtype)
    g_joint = torch.randn((b, p, c), generator=gen).to(dtype)
    worst = {}
    for null in (None, "obj", "quad", "joint"):
        go, gq, gj = (None if null == m else t for m, t in (("obj", g_obj), ("quad", g_quad), ("joint", g_joint)))
        bo, bq, bj, out = IN(go) if p0 > 0 else None, IN(gq) if p0 < p else None, IN(gj), Buf(b * p * c, dtype)
        rc = lib.omnipq_merge_rows(b, p, p0, c, P(bo), P(bq), P(bj), P(out), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = out.get(b, p, c)
        assert all(x is None or x.guards_intact() for x in (bo, bq, bj))
        terms = dr.merge_terms(b, p, p0, c, go, gq, gj, dtype)
        if gj is None:
            assert same_bits(got, terms[0]), null                            # pure data movement
        else:
            tot, bnd = dr.sum_bound(terms, dtype)
            rat = dr.ratios(dict(s=got), dict(s=tot), dict(s=bnd))
            assert not dr.outside(rat), (null, rat)
            assert same_bits(got, (terms[0].float() + terms[1].float()).to(dtype)), null
            worst = rat if not worst or rat["s"][0] > worst["s"][0] else worst
    report(LIB_IDS[LIBS.index(dtype)], f"merge-{b}x{p}x{c}-p0={p0}", worst)
