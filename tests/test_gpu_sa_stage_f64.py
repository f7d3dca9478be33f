"""GPU: the streaming kernels of the training SA stage (csrc/sa_stage.hip) through the C ABI against the float64 reference,
ELEMENT BY ELEMENT.

gather, column statistics, BatchNorm finalize / normalise, max-pool (from Y and from recorded extrema), their backward
(statistics and apply, pooled and dense, single, paired and grouped), the f32 copies of the totals and the three scatter forms
are called directly, in both libraries (bfloat16 and IEEE half), with plan = NULL, on buffers this module lays out itself: every
buffer, input or output, sits between two guard bands and is filled with a NaN pattern beforehand.  Every element a kernel owns
must be finite and inside the bound tests/sa_stage_reference.py derives from the kernel's roundings, or bit-equal where the
reference says so (no exceptions, no norms); every guard element must still hold the pattern; inputs must be unchanged.  The
decisions (ReLU gates, first-maximum rows) are computed exactly in float64, never borrowed from a kernel; the pooled backward
takes its forward pass from the reference.  The chain tests feed each kernel the previous kernel's DEVICE output and evaluate
the reference from those same tensors.  The cases are sa_stage_reference's tables; the CPU suite holds an emulation of the
kernels' arithmetic, and sixteen mutants of it, against the same bounds on the same cases (tests/test_sa_stage_reference.py).

Each test prints `RATIO <library> <case>: <output>=<largest error / bound> ...` (pytest -s); the pass condition is ratio <= 1
on every element.  Largest ratios per library and output over all cases, measured on an MI355X (bfloat16 | half, the case):
    gather        rel     0.664 | 0.661   gather-stride (one e16 rounding: 1 / MARGIN)
    colstats(_z)  sums    0.274 | 0.381   colstats-C640-R2 | -R4     (0.03 - 0.05 on long columns: the bound is a worst case
                                          per addition, the error of n random roundings grows like sqrt n)
    finalize      a 0.548  b 0.361  mean 0.623  invstd 0.632  running_mean 0.473  running_var 0.398   (both libraries alike;
                                          omnipq_bn_finalize, _relu and omnipq_sa_pool_select_finalize publish the same bits)
    normalise     x       0.660 | 0.662   bnrelu-pool-C288 | bnrelu-pool-stride
    pool, pool_select     out_f32 0.000: bit-equal to the f32 rounding of the exact number on every case; arg, ysel, out_pm bits
    dense stats   sums    0.310 | 0.264   dense-stats-C640-R2 | -R4
    pooled stats  sums    0.645 | 0.645   pool-stats-C640-R2 (= sel-stats, sel-hot: two terms, one rounding); hot words: bits
    apply         dY      pooled 0.661 | 0.661   plain 0.656 | 0.655   fused 0.664 | 0.666 (big route; pair and group alike)
    scatter       atomic  dfeat 0.086 | 0.212  dxyz 0.597 | 0.618  dcentre 0.287 | 0.251
                  CSR     dfeat 0.599 | 0.638  dxyz 0.325 | 0.495  dcentre 0.170 | 0.170
                  rows    dfeat32 0.633 | 0.627  dfeat16 0.649 | 0.628  dxyz 0.408 | 0.286  dcentre 0.112 | 0.119
    chains        colstats 0.027 | 0.051, finalize 0.31 - 0.64, dense stats 0.052 | 0.047, pooled stats 0.035, dY 0.66
Nothing is above 1 / MARGIN; the e16 outputs sit at one worst-case store rounding.  No f32 output is below 0.05 on every case:
the statistics reach 0.27 - 0.65 where a column is two or four rows long, and fall to 0.03 - 0.05 on the longest chains.
"""
import ctypes
import sys

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import capi
import sa_stage_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
PATTERN = {torch.float32: (torch.int32, 0x7FC00001), torch.bfloat16: (torch.int16, 0x7FC1), torch.float16: (torch.int16, 0x7E01),
           torch.float64: (torch.int64, 0x7FF8000000000001), torch.uint8: (torch.uint8, 0xA5), torch.int32: (torch.int32, 0x7FC00001)}
LIBS = [torch.bfloat16, torch.float16]
LIB_IDS = ["bf16", "f16"]
NULL = ctypes.c_void_p(0)
F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32
OK, EINVAL = 0, 10001
APPLY_SHAPES = [(16, 1), (24, 17), (128, 37), (288, 8), (640, 4)]


def lib_of(dtype):
    lib, ext = capi.lib_of(dtype)
    if lib is None:
        assert dtype is torch.float16 and ext.LIB_F16_PATH is None
        pytest.skip("no IEEE-half library in this build")
    return lib, ext._stream(0)


def name_of(dtype):
    return LIB_IDS[LIBS.index(dtype)]


class Buf:
    """`numel` elements between two guard bands, all of it the NaN pattern of the type; `data` is copied to the front"""

    def __init__(self, numel, dtype, data=None):
        self.n, self.dtype = numel, dtype
        self.it, self.pat = PATTERN[dtype]
        self.t = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
        self.t.view(self.it).fill_(self.pat)
        self.data = data
        if data is not None:
            assert data.dtype is dtype and data.numel() <= numel, (data.dtype, dtype)
            self.t[GUARD:GUARD + data.numel()].copy_(data.reshape(-1))

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())

    def guards_intact(self):
        b = self.t.view(self.it)
        return bool((b[:GUARD] == self.pat).all()) and bool((b[GUARD + self.n:] == self.pat).all())

    def blank(self):
        """nothing was written at all"""
        return bool((self.t.view(self.it) == self.pat).all())

    def get(self, *shape):
        assert self.guards_intact(), "wrote outside the buffer"
        return self.t[GUARD:GUARD + self.n].cpu().reshape(*shape)

    def unchanged(self):
        return self.guards_intact() and torch.equal(sr.bits(self.get(-1)[:self.data.numel()]), sr.bits(self.data.reshape(-1)))


def P(buf):
    return NULL if buf is None else buf.ptr()


def IN(t):
    return None if t is None else Buf(t.numel(), t.dtype, t.contiguous())


def ins(inp, *names):
    return {n: IN(inp[n]) for n in names}


def all_unchanged(bufs):
    for n, b in bufs.items():
        assert b is None or b.unchanged(), f"input {n} was modified"


def run(rc):
    assert rc == OK, rc
    torch.cuda.synchronize()


def report(dtype, id, got, ref, expect=None):
    """ref = (want, bounds, exact).  Prints the RATIO line and asserts that nothing is outside."""
    for n, g in got.items():
        assert g.dtype in (U8, I32) or bool(torch.isfinite(g.double()).all()), (id, n, "not finite")
    rat, broken = sr.verdict(got, *ref)
    if expect is not None:
        assert set(got) == set(expect), (set(got), expect)
    print(f"\n  RATIO {name_of(dtype)} {id}: {sr.fmt(rat)}" + "".join(f" {n}=bits" for n in ref[2] if n in got))
    assert not broken, (name_of(dtype), id, broken, sr.fmt(rat))


# ---- gather ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("case", sr.GATHER_CASES, ids=[c["id"] for c in sr.GATHER_CASES])
def test_gather(case, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.gather_inputs(case, dtype)
    b, n, m, s, cin, kpad = (case[k] for k in ("b", "n", "m", "s", "cin", "kpad"))
    rows = b * m * s
    bufs = ins(inp, "xyz", "centre", "idx")
    bufs["feat"] = IN(inp["feat"]) if cin else None
    X = Buf(rows * kpad, dtype)
    run(lib.omnipq_sa_gather(b, n, m, s, cin, kpad, inp["inv_r"], P(bufs["xyz"]), P(bufs["centre"]), P(bufs["idx"]), P(bufs["feat"]),
                             P(X), NULL, stream))
    all_unchanged(bufs)
    report(dtype, case["id"], sr.split_gathered(X.get(rows, kpad), cin), sr.gather_reference(inp, dtype),
           expect=("feat_cols", "rel", "pad_cols"))


# ---- column statistics ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("C,rows", sr.STATS_SHAPES)
def test_colstats_overwrites_and_colstats_z_adds(C, rows, dtype):
    lib, stream = lib_of(dtype)
    for z in (False, True):
        inp = sr.colstats_inputs(C, rows, dtype, sums0=z)
        y = IN(inp["y"])
        sums = Buf(2 * C, F64, inp["sums0"])                 # plain: the NaN pattern, which the call has to clear
        run((lib.omnipq_colstats_z if z else lib.omnipq_colstats)(rows, C, P(y), P(sums), stream))
        assert y.unchanged()
        report(dtype, f"colstats{'_z' if z else ''}-C{C}-R{rows}", dict(sums=sums.get(2, C)), sr.colstats_reference(inp))


# ---- finalize -------------------------------------------------------------------------------------------------------------

FIN_OUT = ("a", "b", "mean", "invstd")


def _finalize_call(lib, stream, inp, entry, dtype, y=None):
    """entry: "plain", "relu" (Y -> X with it) or "select" (the extrema of Y -> the pooled outputs with it).
    -> (got of the finalize, extra buffers, inputs)"""
    C = inp["C"]
    bufs = ins(inp, "sums", "gamma", "beta", "bias")
    run_m, run_v = (Buf(C, F32, inp["rm"]), Buf(C, F32, inp["rv"])) if inp["rm"] is not None else (None, None)
    out = {n: Buf(C, F32) for n in FIN_OUT}
    extra = {}
    if entry == "plain":
        rc = lib.omnipq_bn_finalize(C, inp["cnt"], P(bufs["sums"]), P(bufs["gamma"]), P(bufs["beta"]), inp["eps"], inp["mom"], P(run_m),
                                    P(run_v), P(out["a"]), P(out["b"]), P(out["mean"]), P(out["invstd"]), P(bufs["bias"]), stream)
    elif entry == "relu":
        rows = y.shape[0]
        bufs["Y"] = IN(y)
        extra["X"] = Buf(rows * C, dtype)
        rc = lib.omnipq_bn_finalize_relu(rows, C, inp["cnt"], P(bufs["sums"]), P(bufs["gamma"]), P(bufs["beta"]), inp["eps"], inp["mom"],
                                         P(run_m), P(run_v), P(bufs["bias"]), P(bufs["Y"]), P(extra["X"]), P(out["a"]), P(out["b"]),
                                         P(out["mean"]), P(out["invstd"]), stream)
    else:
        BM = y.shape[0]
        ext = dict(zip(("ymax", "ymin", "amax", "amin"), sr.extrema(y)))
        bufs.update({n: IN(t) for n, t in ext.items()})
        extra = dict(out_f32=Buf(BM * C, F32), out_pm=Buf(BM * C, dtype), arg=Buf(BM * C, U8), ysel=Buf(BM * C, dtype))
        rc = lib.omnipq_sa_pool_select_finalize(BM, C, P(bufs["ymax"]), P(bufs["ymin"]), P(bufs["amax"]), P(bufs["amin"]), P(bufs["sums"]),
                                                inp["cnt"], P(bufs["gamma"]), P(bufs["beta"]), inp["eps"], inp["mom"], P(run_m), P(run_v),
                                                P(out["a"]), P(out["b"]), P(out["mean"]), P(out["invstd"]), P(extra["out_f32"]),
                                                P(extra["out_pm"]), P(extra["arg"]), P(extra["ysel"]), NULL, stream)
    run(rc)
    all_unchanged(bufs)
    got = {n: out[n].get(C) for n in FIN_OUT}
    if run_m is not None:
        got.update(rm=run_m.get(C), rv=run_v.get(C))
    return got, extra


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("entry", ["plain", "relu", "select"])
@pytest.mark.parametrize("case", sr.FINALIZE_CASES, ids=[c["id"] for c in sr.FINALIZE_CASES])
def test_finalize(case, entry, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.finalize_inputs(case)
    if entry == "select":
        inp["bias"] = None                                   # (omnipq_sa_pool_select_finalize knows no conv bias)
    C = inp["C"]
    gen = torch.Generator().manual_seed(C)
    y = sr.dy(gen, (5, 3, C), -6, 3).to(dtype)               # five balls of three rows / fifteen rows
    y[1, 1:] = y[1, 0]
    got, extra = _finalize_call(lib, stream, inp, entry, dtype, y=y.reshape(15, C) if entry == "relu" else y)
    report(dtype, f"{entry}-{case['id']}", got, sr.finalize_reference(inp),
           expect=FIN_OUT + (("rm", "rv") if case["running"] else ()))
    # what the launch did with the constants it derived: the reference from the PUBLISHED a, b.  The sign of a y + b is that
    # of its float64 value for any f32 a, b (the product is exact, a float64 sum keeps the sign of the exact one)
    dev = dict(Y=y, a=got["a"], b=got["b"])
    if entry == "relu":
        report(dtype, f"relu-x-{case['id']}", dict(x=extra["X"].get(5, 3, C)), sr.bnrelu_reference(dev, dtype))
    elif entry == "select":
        sel = dict(out_f32=extra["out_f32"].get(5, C), out_pm=extra["out_pm"].get(5, C), arg=extra["arg"].get(5, C),
                   ysel=extra["ysel"].get(5, C))
        report(dtype, f"select-out-{case['id']}", sel, sr.pool_select_reference(dev, dtype, got=sel))


# ---- normalise, pool, pool_select -------------------------------------------------------------------------------------------

def _pool_call(lib, stream, inp, dtype, select):
    BM, s, C = inp["Y"].shape
    bufs = ins(inp, "a", "b")
    out = dict(out_f32=Buf(BM * C, F32), out_pm=Buf(BM * C, dtype), arg=Buf(BM * C, U8))
    if select:
        out["ysel"] = Buf(BM * C, dtype)
        bufs.update({n: IN(t) for n, t in zip(("ymax", "ymin", "amax", "amin"), sr.extrema(inp["Y"]))})   # from the reference
        rc = lib.omnipq_sa_pool_select(BM, C, P(bufs["ymax"]), P(bufs["ymin"]), P(bufs["amax"]), P(bufs["amin"]), P(bufs["a"]),
                                       P(bufs["b"]), P(out["out_f32"]), P(out["out_pm"]), P(out["arg"]), P(out["ysel"]), stream)
    else:
        bufs["Y"] = IN(inp["Y"])
        rc = lib.omnipq_sa_pool(1, BM, s, C, P(bufs["Y"]), P(bufs["a"]), P(bufs["b"]), P(out["out_f32"]), P(out["out_pm"]),
                                P(out["arg"]), stream)
    run(rc)
    all_unchanged(bufs)
    return {n: o.get(BM, C) for n, o in out.items()}


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("case", sr.POOL_CASES, ids=[c["id"] for c in sr.POOL_CASES])
def test_normalise_pool_and_pool_select(case, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.pool_inputs(case, dtype)
    BM, s, C = inp["Y"].shape
    bufs = ins(inp, "Y", "a", "b")
    X = Buf(BM * s * C, dtype)
    run(lib.omnipq_bnrelu(BM * s, C, P(bufs["Y"]), P(bufs["a"]), P(bufs["b"]), P(X), stream))
    all_unchanged(bufs)
    report(dtype, f"bnrelu-{case['id']}", dict(x=X.get(BM, s, C)), sr.bnrelu_reference(inp, dtype))
    got = _pool_call(lib, stream, inp, dtype, select=False)
    report(dtype, f"pool-{case['id']}", got, sr.pool_reference(inp, dtype, got=got), expect=("out_f32", "out_pm", "arg"))
    got = _pool_call(lib, stream, inp, dtype, select=True)
    report(dtype, f"select-{case['id']}", got, sr.pool_select_reference(inp, dtype, got=got),
           expect=("out_f32", "out_pm", "arg", "ysel"))
    if case["gated"]:
        assert not bool(got["out_f32"].any()) and not bool(got["arg"].any())


# ---- backward statistics ----------------------------------------------------------------------------------------------------

def _dense_stats(lib, stream, inp, z, sums=None):
    rows, C = inp["Y"].shape
    bufs = ins(inp, "dX", "Y", "a", "b", "mean", "invstd")
    sums = Buf(3 * C, F64, inp.get("sums0")) if sums is None else sums
    fn = lib.omnipq_bn_bwd_stats_z if z else lib.omnipq_bn_bwd_stats
    run(fn(rows, C, P(bufs["dX"]), P(bufs["Y"]), P(bufs["a"]), P(bufs["b"]), P(bufs["mean"]), P(bufs["invstd"]), P(sums), stream))
    all_unchanged(bufs)
    return sums


def _third_row_untouched(sums, C):
    return bool((sums.t.view(torch.int64)[GUARD + 2 * C:GUARD + 3 * C] == sums.pat).all())


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("C,rows", sr.STATS_SHAPES)
def test_dense_backward_statistics(C, rows, dtype):
    lib, stream = lib_of(dtype)
    for z in (False, True):
        inp = sr.dense_inputs(C, rows, dtype)
        if z:
            inp["sums0"] = torch.arange(2 * C, dtype=F64).reshape(2, C) / 7.0 - 3.0
        sums = _dense_stats(lib, stream, inp, z)
        assert _third_row_untouched(sums, C)
        report(dtype, f"dense-stats{'_z' if z else ''}-C{C}-R{rows}", dict(sums=sums.get(3, C)[:2]),
               sr.bwd_stats_reference(inp, "dense"))


def _pool_stats(lib, stream, inp, entry, dtype, zeroed=0):
    """entry: "pool" (gathers y from Y), "sel", "hot".  -> (sums Buf, hot Buf | None)"""
    BM, s, C = inp["Y"].shape
    names = ("mean", "invstd", "g_out", "out_pm") + (("Y", "arg") if entry == "pool" else ("ysel",)) + \
            (("a", "arg") if entry == "hot" else ())
    bufs = ins(inp, *names)
    sums, hot = Buf(3 * C, F64, inp.get("sums0")), None
    if entry == "pool":
        rc = lib.omnipq_sa_pool_bwd_stats(1, BM, s, C, P(bufs["Y"]), P(bufs["mean"]), P(bufs["invstd"]), P(bufs["g_out"]),
                                          P(bufs["out_pm"]), P(bufs["arg"]), P(sums), stream)
    elif entry == "sel":
        rc = lib.omnipq_sa_pool_bwd_stats_sel(BM, C, P(bufs["ysel"]), P(bufs["mean"]), P(bufs["invstd"]), P(bufs["g_out"]),
                                              P(bufs["out_pm"]), P(sums), zeroed, stream)
    else:
        hot = Buf(BM * C, I32)
        rc = lib.omnipq_sa_pool_bwd_stats_sel_hot(BM, C, P(bufs["ysel"]), P(bufs["mean"]), P(bufs["invstd"]), P(bufs["g_out"]),
                                                  P(bufs["out_pm"]), P(sums), zeroed, P(bufs["a"]), P(bufs["arg"]), P(hot), stream)
    run(rc)
    all_unchanged(bufs)
    assert _third_row_untouched(sums, C)
    return sums, hot


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("C,BM", sr.STATS_SHAPES)
def test_pooled_backward_statistics(C, BM, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.pool_stats_inputs(C, BM, dtype, select=False)
    sums, _ = _pool_stats(lib, stream, inp, "pool", dtype)
    report(dtype, f"pool-stats-C{C}-R{BM}", dict(sums=sums.get(3, C)[:2]), sr.bwd_stats_reference(inp, "pool"))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("C,BM", sr.SEL_SHAPES)
def test_selected_backward_statistics_and_hot_words(C, BM, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.pool_stats_inputs(C, BM, dtype, select=True)
    sums, _ = _pool_stats(lib, stream, inp, "sel", dtype)
    report(dtype, f"sel-stats-C{C}-R{BM}", dict(sums=sums.get(3, C)[:2]), sr.bwd_stats_reference(inp, "sel"))
    inp["sums0"] = torch.arange(2 * C, dtype=F64).reshape(2, C) / 5.0 - 2.0           # zeroed != 0: the totals are ADDED
    sums, hot = _pool_stats(lib, stream, inp, "hot", dtype, zeroed=1)
    want, bnd, _ = sr.bwd_stats_reference(inp, "sel")
    report(dtype, f"sel-hot-C{C}-R{BM}", dict(sums=sums.get(3, C)[:2], hot=hot.get(BM, C)),
           (want, bnd, dict(hot=sr.hot_words(inp, dtype))), expect=("sums", "hot"))


# ---- backward apply ---------------------------------------------------------------------------------------------------------

# every pool case of at most 64 balls; two of them also in the process-group use: 2 P positions, doubled totals
POOLED_APPLY = [(c, 1.0) for c in sr.POOL_CASES if c["BM"] <= 64] + [(sr.by_id(sr.POOL_CASES, id), 2.0) for id in ("pool-s5", "pool-C640")]


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("case,scale", POOLED_APPLY, ids=[f"{c['id']}-x{k:g}" for c, k in POOLED_APPLY])
def test_pooled_backward_apply(case, scale, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.pool_stats_inputs(case["C"], case["BM"], dtype, select=False, s=case["s"])
    BM, s, C = inp["Y"].shape
    totals = sr.exact_totals(inp, "pool", scale)
    total = scale * BM * s
    for gb in (False, True):
        bufs = ins(inp, "Y", "a", "mean", "invstd", "g_out", "out_pm", "arg")
        bufs["sums"] = Buf(3 * C, F64, totals)
        dY, gbo = Buf(BM * s * C, dtype), Buf(2 * C, F32)
        args = (1, BM, s, C, total, P(bufs["Y"]), P(bufs["a"]), P(bufs["mean"]), P(bufs["invstd"]), P(bufs["sums"]), P(bufs["g_out"]),
                P(bufs["out_pm"]), P(bufs["arg"]), P(dY))
        run(lib.omnipq_sa_pool_bwd_apply_gb(*args, P(gbo), NULL, stream) if gb else lib.omnipq_sa_pool_bwd_apply(*args, NULL, stream))
        all_unchanged(bufs)
        assert _third_row_untouched(bufs["sums"], C)
        got = dict(dY=dY.get(BM, s, C))
        if gb:
            got["gb"] = gbo.get(2, C)
        else:
            assert gbo.blank()
        report(dtype, f"apply{'_gb' if gb else ''}-{case['id']}-x{scale:g}", got,
               sr.apply_reference(inp, "pool", totals, total, dtype, "pool"), expect=("dY", "gb") if gb else ("dY",))


def _fused(lib, stream, inp, totals, total, dtype, dbg):
    """issues omnipq_bn_bwd_apply_fused.  -> (input buffers, dY, dbeta_dgamma | None)"""
    rows, C = inp["Y"].shape
    bufs = ins(inp, "dX", "Y", "a", "b", "mean", "invstd")
    bufs["sums"] = Buf(2 * C, F64, totals)
    dY, out = Buf(rows * C, dtype), (Buf(2 * C, F32) if dbg else None)
    rc = lib.omnipq_bn_bwd_apply_fused(rows, C, total, P(bufs["dX"]), P(bufs["Y"]), P(bufs["a"]), P(bufs["b"]), P(bufs["mean"]),
                                       P(bufs["invstd"]), P(bufs["sums"]), P(dY), P(out), NULL, stream)
    assert rc == OK, rc
    return bufs, dY, out


def _fused_result(held, inp):
    bufs, dY, out = held
    all_unchanged(bufs)
    got = dict(dY=dY.get(*inp["Y"].shape))
    if out is not None:
        got["gb"] = out.get(2, inp["Y"].shape[1])
    return got


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("scale", [1.0, 2.0], ids=["own", "group"])
@pytest.mark.parametrize("C,rows", APPLY_SHAPES)
def test_dense_backward_apply_plain_and_fused(C, rows, scale, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.dense_inputs(C, rows, dtype)
    totals, total = sr.exact_totals(inp, "dense", scale), scale * rows
    bufs = ins(inp, "dX", "Y", "a", "b", "mean", "invstd")
    sums, dY = Buf(3 * C, F64, totals), Buf(rows * C, dtype)
    run(lib.omnipq_bn_bwd_apply(rows, C, total, P(bufs["dX"]), P(bufs["Y"]), P(bufs["a"]), P(bufs["b"]), P(bufs["mean"]),
                                P(bufs["invstd"]), P(sums), P(dY), stream))
    all_unchanged(bufs)
    assert sums.unchanged(), "the totals (rows 0, 1 of sums) were modified"      # row 2 is scratch: anything may be there
    report(dtype, f"apply-plain-C{C}-R{rows}-x{scale:g}", dict(dY=dY.get(rows, C)),
           sr.apply_reference(inp, "dense", totals, total, dtype, "plain"), expect=("dY",))
    for dbg in (False, True):
        held = _fused(lib, stream, inp, totals, total, dtype, dbg)
        torch.cuda.synchronize()
        report(dtype, f"apply-fused{'-dbg' if dbg else ''}-C{C}-R{rows}-x{scale:g}", _fused_result(held, inp),
               sr.apply_reference(inp, "dense", totals, total, dtype, "fused"), expect=("dY", "gb") if dbg else ("dY",))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_fused_apply_big_route(dtype):
    """P = 32776, C = 256: 2^20 + 256 pieces -- four per thread, non-temporal loads, a last workgroup that is mostly idle"""
    lib, stream = lib_of(dtype)
    inp = sr.dense_inputs(sr.BIG_C, sr.BIG_P, dtype)
    totals = sr.exact_totals(inp, "dense")
    held = _fused(lib, stream, inp, totals, float(sr.BIG_P), dtype, True)
    torch.cuda.synchronize()
    report(dtype, "apply-fused-big", _fused_result(held, inp),
           sr.apply_reference(inp, "dense", totals, float(sr.BIG_P), dtype, "fused"), expect=("dY", "gb"))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("n", [2, 3], ids=["pair", "group3"])
def test_fused_apply_paired_and_grouped(n, dtype):
    """omnipq_pair_hold / omnipq_pair_group: members of different C and P in ONE grid, each against the reference"""
    lib, stream = lib_of(dtype)
    shapes = [(288, 8), (24, 17), (128, 37)][:n]
    inps = [sr.dense_inputs(C, rows, dtype) for C, rows in shapes]
    totals = [sr.exact_totals(inp, "dense") for inp in inps]
    before = int(lib.omnipq_pair_flush())
    if n > 2:
        assert lib.omnipq_pair_group(n) == OK
    held = []
    for i, (inp, tot) in enumerate(zip(inps, totals)):
        if i < n - 1:
            lib.omnipq_pair_hold()
        held.append(_fused(lib, stream, inp, tot, float(inp["Y"].shape[0]), dtype, dbg=i != 1))
        assert lib.omnipq_pair_held() == (i + 1 if i < n - 1 else 0)
    assert int(lib.omnipq_pair_flush()) - before == 1, "the members did not share a grid"
    torch.cuda.synchronize()
    for i, (inp, tot, h) in enumerate(zip(inps, totals, held)):
        report(dtype, f"apply-fused-{'pair' if n == 2 else 'group3'}-member{i}", _fused_result(h, inp),
               sr.apply_reference(inp, "dense", tot, float(inp["Y"].shape[0]), dtype, "fused"),
               expect=("dY", "gb") if i != 1 else ("dY",))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("C", [8, 24, 136, 640])
def test_sums_to_f32(C, dtype):
    lib, stream = lib_of(dtype)
    gen = torch.Generator().manual_seed(C)
    totals = torch.randn((2, C), generator=gen, dtype=F64) * 10.0 ** (8 * torch.rand((2, C), generator=gen, dtype=F64) - 4)
    sums, dbeta, dgamma = Buf(2 * C, F64, totals), Buf(C, F32), Buf(C, F32)
    run(lib.omnipq_sums_to_f32(C, P(sums), P(dbeta), P(dgamma), stream))
    assert sums.unchanged()
    report(dtype, f"sums_to_f32-C{C}", dict(gb=torch.stack([dbeta.get(C), dgamma.get(C)])), ({}, {}, dict(gb=totals.to(F32))))


# ---- scatter ----------------------------------------------------------------------------------------------------------------

def _zeros(numel):
    return Buf(numel, F32, torch.zeros(numel))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("case", sr.SCATTER_CASES, ids=[c["id"] for c in sr.SCATTER_CASES])
def test_scatter_atomic_and_csr(case, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.scatter_inputs(case, dtype)
    b, n, m, s, cin, kpad = (case[k] for k in ("b", "n", "m", "s", "cin", "kpad"))

    def outputs(make):
        return (make(b * n * cin) if case["dfeat"] and cin else None, make(b * n * 3) if case["dxyz"] else None,
                make(b * m * 3) if case["dxyz"] else None)

    def collect(dfeat, dxyz, dcen):
        got = {}
        if dfeat is not None:
            got["dfeat"] = dfeat.get(b * n, cin)
        if dxyz is not None:
            got.update(dxyz=dxyz.get(b * n, 3), dcentre=dcen.get(b * m, 3))
        return got

    bufs = ins(inp, "idx", "dX")
    outs = outputs(_zeros)                                   # the atomic form ADDS: zero-initialised outputs
    run(lib.omnipq_sa_scatter(b, n, m, s, cin, kpad, inp["inv_r"], P(bufs["idx"]), P(bufs["dX"]), *[P(o) for o in outs], stream))
    all_unchanged(bufs)
    ref = sr.scatter_reference(dict(inp, dfeat=case["dfeat"] and cin > 0), dtype, "atomic")
    report(dtype, f"atomic-{case['id']}", collect(*outs), ref, expect=set(ref[0]))
    # the CSR form writes every entry: outputs start as the NaN pattern.  One case takes its CSR from omnipq_sa_build_csr
    if case["id"] == "scatter-long":
        offsets, order, scratch = Buf(b * (n + 1), I32), Buf(b * m * s, I32), Buf(b * n, I32)
        run(lib.omnipq_sa_build_csr(b, n, m, s, P(bufs["idx"]), P(offsets), P(order), P(scratch), NULL, stream))
        assert torch.equal(offsets.get(b, n + 1), inp["offsets"])
        dev_order = order.get(b, m * s)
        for i in range(b):                                   # the same buckets, in whatever order inside a bucket
            for k in range(n):
                lo, hi = int(inp["offsets"][i, k]), int(inp["offsets"][i, k + 1])
                assert torch.equal(dev_order[i, lo:hi].sort().values, inp["order"][i, lo:hi])
        bufs.update(offsets=offsets, order=order)
    else:
        bufs.update(ins(inp, "offsets", "order"))
    outs = outputs(lambda numel: Buf(numel, F32))
    run(lib.omnipq_sa_scatter_csr(b, n, m, s, cin, kpad, inp["inv_r"], P(bufs["offsets"]), P(bufs["order"]), P(bufs["dX"]),
                                  *[P(o) for o in outs], NULL, stream))
    assert bufs["dX"].unchanged() and bufs["offsets"].guards_intact() and bufs["order"].guards_intact()
    ref = sr.scatter_reference(dict(inp, dfeat=case["dfeat"] and cin > 0), dtype, "csr")
    report(dtype, f"csr-{case['id']}", collect(*outs), ref, expect=set(ref[0]))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("case", sr.ROWS_CASES, ids=[c["id"] for c in sr.ROWS_CASES])
def test_scatter_rows_csr(case, dtype):
    lib, stream = lib_of(dtype)
    inp = sr.scatter_inputs(case, dtype, rows_form=True)
    b, n, m, s, C = (case[k] for k in ("b", "n", "m", "s", "cin"))
    ref = sr.scatter_reference(inp, dtype, "rows")
    for which in ("both", "f32", "e16"):
        bufs = ins(inp, "offsets", "order", "dY", "dXr")
        d32 = Buf(b * n * C, F32) if which != "e16" else None
        d16 = Buf(b * n * C, dtype) if which != "f32" else None
        dxyz, dcen = (Buf(b * n * 3, F32), Buf(b * m * 3, F32)) if case["dxyz"] else (None, None)
        run(lib.omnipq_sa_scatter_rows_csr(b, n, m, s, C, inp["inv_r"], P(bufs["offsets"]), P(bufs["order"]), P(bufs["dY"]),
                                           P(bufs["dXr"]), NULL, 0, P(d32), P(d16), P(dxyz), P(dcen), stream))
        all_unchanged(bufs)
        got = {}
        if d32 is not None:
            got["dfeat32"] = d32.get(b * n, C)
        if d16 is not None:
            got["dfeat16"] = d16.get(b * n, C)
        if dxyz is not None:
            got.update(dxyz=dxyz.get(b * n, 3), dcentre=dcen.get(b * m, 3))
        report(dtype, f"{case['id']}-{which}", got, ref)
        assert set(got) == set(ref[0]) - ({"dfeat32"} if which == "e16" else set()) - ({"dfeat16"} if which == "f32" else set())


# ---- chains: every kernel is fed the previous kernel's DEVICE output ----------------------------------------------------------

def _chain_forward_inputs(dtype):
    """37 balls of 5 rows, 24 channels; gamma / beta chosen so that the a, b the DEVICE derives fall into the exact ranges"""
    gen = torch.Generator().manual_seed(77)
    BM, s, C = 37, 5, 24
    y = sr.pad_balls(gen, sr.y_rows(gen, BM * s, C, dtype).reshape(BM, s, C), s)
    gamma = torch.sign(torch.randn(C, generator=gen)) * (0.5 + torch.rand(C, generator=gen))
    beta = torch.sign(torch.randn(C, generator=gen)) * (0.75 + 0.5 * torch.rand(C, generator=gen))
    gamma[5], beta[5] = 0.125, 13.0                         # mean 6, invstd 16: a = 2, b = 13 - 12
    gamma[6], beta[6] = 2.0 ** -8, 0.0                      # constant 1.25: invstd = eps^-1/2 = 316
    return y, dict(C=C, cnt=float(BM * s), gamma=gamma, beta=beta, eps=sr.as_f32(sr.EPS), mom=sr.as_f32(0.1),
                   rm=torch.randn(C, generator=gen), rv=torch.rand(C, generator=gen) + 0.5, bias=torch.randn(C, generator=gen))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_forward_chain(dtype):
    """statistics -> finalize -> normalise and pool; the reference of each step from the tensors the step read"""
    lib, stream = lib_of(dtype)
    y, fin = _chain_forward_inputs(dtype)
    BM, s, C = y.shape
    yb, sums = IN(y), Buf(2 * C, F64)
    run(lib.omnipq_colstats(BM * s, C, P(yb), P(sums), stream))
    dev_sums = sums.get(2, C)
    report(dtype, "chain-colstats", dict(sums=dev_sums), sr.colstats_reference(dict(y=y.reshape(BM * s, C), sums0=None)))
    fin["sums"] = dev_sums
    got, _ = _finalize_call(lib, stream, fin, "plain", dtype)
    report(dtype, "chain-finalize", got, sr.finalize_reference(fin))
    dev = dict(Y=y, a=got["a"], b=got["b"])
    assert sr.in_exact_ranges(dev["a"], dev["b"], y), "the chain's constants left the ranges in which a y + b is exact"
    bufs = ins(dev, "Y", "a", "b")
    X = Buf(BM * s * C, dtype)
    run(lib.omnipq_bnrelu(BM * s, C, P(bufs["Y"]), P(bufs["a"]), P(bufs["b"]), P(X), stream))
    report(dtype, "chain-bnrelu", dict(x=X.get(BM, s, C)), sr.bnrelu_reference(dev, dtype))
    pooled = _pool_call(lib, stream, dev, dtype, select=False)
    report(dtype, "chain-pool", pooled, sr.pool_reference(dev, dtype, got=pooled))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_backward_chains(dtype):
    """backward statistics -> apply, dense (fused) and pooled, the device totals fed on"""
    lib, stream = lib_of(dtype)
    inp = sr.dense_inputs(288, 3585, dtype)
    rows, C = inp["Y"].shape
    sums = _dense_stats(lib, stream, inp, False)
    dev_tot = sums.get(3, C)[:2].clone()
    report(dtype, "chain-dense-stats", dict(sums=dev_tot), sr.bwd_stats_reference(inp, "dense"))
    held = _fused(lib, stream, inp, dev_tot, float(rows), dtype, True)
    torch.cuda.synchronize()
    report(dtype, "chain-dense-apply", _fused_result(held, inp), sr.apply_reference(inp, "dense", dev_tot, float(rows), dtype, "fused"))
    inp = sr.pool_stats_inputs(24, 37, dtype, select=False, s=5)
    BM, s, C = inp["Y"].shape
    sums, _ = _pool_stats(lib, stream, inp, "pool", dtype)
    dev_tot = sums.get(3, C)[:2].clone()
    report(dtype, "chain-pool-stats", dict(sums=dev_tot), sr.bwd_stats_reference(inp, "pool"))
    bufs = ins(inp, "Y", "a", "mean", "invstd", "g_out", "out_pm", "arg")
    dY, gbo = Buf(BM * s * C, dtype), Buf(2 * C, F32)
    run(lib.omnipq_sa_pool_bwd_apply_gb(1, BM, s, C, float(BM * s), P(bufs["Y"]), P(bufs["a"]), P(bufs["mean"]), P(bufs["invstd"]),
                                        P(sums), P(bufs["g_out"]), P(bufs["out_pm"]), P(bufs["arg"]), P(dY), P(gbo), NULL, stream))
    report(dtype, "chain-pool-apply", dict(dY=dY.get(BM, s, C), gb=gbo.get(2, C)),
           sr.apply_reference(inp, "pool", dev_tot, float(BM * s), dtype, "pool"))


# ---- the argument table -------------------------------------------------------------------------------------------------------

class Arena:
    """buffers of one argument-table entry: whatever a call writes shows as a buffer that is no longer blank"""

    def __init__(self):
        self.bufs = []

    def new(self, numel, dtype):
        self.bufs.append(Buf(numel, dtype))
        self.bufs[-1].line = sys._getframe(2).f_lineno       # the table row that asked for it
        return self.bufs[-1].ptr()

    def touched(self):
        """[(line of the call, type)] of the buffers that no longer hold the pattern"""
        torch.cuda.synchronize()
        return [(b.line, b.dtype) for b in self.bufs if not b.blank()]


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_argument_table(dtype):
    """EINVAL and OK-on-nothing without a single write: every pointer below is a NaN-pattern buffer, blank afterwards"""
    lib, stream = lib_of(dtype)
    ar = Arena()
    N = 16384

    def p(dt=F32):
        return ar.new(N, dt)

    def e():
        return p(dtype)

    def stats_calls(C, rows):
        return [("colstats", lib.omnipq_colstats(rows, C, e(), p(F64), stream)),
                ("colstats_z", lib.omnipq_colstats_z(rows, C, e(), p(F64), stream)),
                ("bn_bwd_stats", lib.omnipq_bn_bwd_stats(rows, C, e(), e(), p(), p(), p(), p(), p(F64), stream)),
                ("bn_bwd_stats_z", lib.omnipq_bn_bwd_stats_z(rows, C, e(), e(), p(), p(), p(), p(), p(F64), stream)),
                ("pool_bwd_stats", lib.omnipq_sa_pool_bwd_stats(1, rows, 2, C, e(), p(), p(), p(), e(), p(U8), p(F64), stream)),
                ("pool_bwd_stats_sel", lib.omnipq_sa_pool_bwd_stats_sel(rows, C, e(), p(), p(), p(), e(), p(F64), 0, stream)),
                ("pool_bwd_stats_sel_hot", lib.omnipq_sa_pool_bwd_stats_sel_hot(rows, C, e(), p(), p(), p(), e(), p(F64), 0, p(), p(U8),
                                                                                p(I32), stream))]

    def streaming_calls(C, rows=2, s=2, b=1, csr=True):
        calls = [("gather", lib.omnipq_sa_gather(b, 5, rows, s, C, C + 8, 1.0, p(), p(), p(I32), e(), e(), NULL, stream)),
                ("bnrelu", lib.omnipq_bnrelu(rows * b, C, e(), p(), p(), e(), stream)),
                ("pool", lib.omnipq_sa_pool(b, rows, s, C, e(), p(), p(), p(), e(), p(U8), stream)),
                ("pool_select", lib.omnipq_sa_pool_select(rows * b, C, e(), e(), p(U8), p(U8), p(), p(), p(), e(), p(U8), e(), stream)),
                ("pool_bwd_apply", lib.omnipq_sa_pool_bwd_apply(b, rows, s, C, 4.0, e(), p(), p(), p(), p(F64), p(), e(), p(U8), e(),
                                                                NULL, stream)),
                ("bn_bwd_apply", lib.omnipq_bn_bwd_apply(rows * b, C, 2.0, e(), e(), p(), p(), p(), p(), p(F64), e(), stream)),
                ("scatter", lib.omnipq_sa_scatter(b, 5, rows, s, C, C + 8, 1.0, p(I32), e(), p(), p(), p(), stream))]
        if not csr:
            return calls
        return calls + [
                ("scatter_csr", lib.omnipq_sa_scatter_csr(b, 5, rows, s, C, C + 8, 1.0, p(I32), p(I32), e(), p(), p(), p(), NULL, stream)),
                ("scatter_rows_csr", lib.omnipq_sa_scatter_rows_csr(b, 5, rows, s, C, 1.0, p(I32), p(I32), e(), e(), NULL, 0, p(), e(),
                                                                    p(), p(), stream))]

    table = []
    table += [(f"{n} C=12", rc, EINVAL) for n, rc in stats_calls(12, 4) + streaming_calls(12)]          # C % 8 != 0
    table += [(f"{n} C={C}", rc, EINVAL) for C in (8, 648) for n, rc in stats_calls(C, 4)]              # below / above the fold
    # (only the entries that must refuse s = 256 are called with it: one that accepts the shape would run on pattern-filled indices)
    table += [("pool s=256", lib.omnipq_sa_pool(1, 2, 256, 16, e(), p(), p(), p(), e(), p(U8), stream), EINVAL),
              ("pool_bwd_apply s=256", lib.omnipq_sa_pool_bwd_apply(1, 2, 256, 16, 4.0, e(), p(), p(), p(), p(F64), p(), e(), p(U8), e(),
                                                                    NULL, stream), EINVAL)]
    table += [("pool_bwd_stats s=256", lib.omnipq_sa_pool_bwd_stats(1, 2, 256, 16, e(), p(), p(), p(), e(), p(U8), p(F64), stream), EINVAL)]
    # NULL required pointers
    table += [("colstats Y=NULL", lib.omnipq_colstats(4, 16, NULL, p(F64), stream), EINVAL),
              ("colstats sums=NULL", lib.omnipq_colstats(4, 16, e(), NULL, stream), EINVAL),
              ("bn_finalize a=NULL", lib.omnipq_bn_finalize(16, 4.0, p(F64), p(), p(), 1e-5, 0.1, NULL, NULL, NULL, p(), p(), p(), NULL,
                                                            stream), EINVAL),
              ("bn_finalize_relu X=NULL", lib.omnipq_bn_finalize_relu(2, 16, 2.0, p(F64), p(), p(), 1e-5, 0.1, NULL, NULL, NULL, e(), NULL,
                                                                      p(), p(), p(), p(), stream), EINVAL),
              ("bnrelu a=NULL", lib.omnipq_bnrelu(2, 16, e(), NULL, p(), e(), stream), EINVAL),
              ("pool arg=NULL", lib.omnipq_sa_pool(1, 2, 2, 16, e(), p(), p(), p(), e(), NULL, stream), EINVAL),
              ("pool_select ysel=NULL", lib.omnipq_sa_pool_select(2, 16, e(), e(), p(U8), p(U8), p(), p(), p(), e(), p(U8), NULL, stream),
               EINVAL),
              ("bn_bwd_stats mean=NULL", lib.omnipq_bn_bwd_stats(4, 16, e(), e(), p(), p(), NULL, p(), p(F64), stream), EINVAL),
              ("pool_bwd_stats_sel_hot hot=NULL", lib.omnipq_sa_pool_bwd_stats_sel_hot(4, 16, e(), p(), p(), p(), e(), p(F64), 0, p(),
                                                                                       p(U8), NULL, stream), EINVAL),
              ("pool_bwd_apply_gb gb=NULL", lib.omnipq_sa_pool_bwd_apply_gb(1, 2, 2, 16, 4.0, e(), p(), p(), p(), p(F64), p(), e(), p(U8),
                                                                            e(), NULL, NULL, stream), EINVAL),
              ("bn_bwd_apply dY=NULL", lib.omnipq_bn_bwd_apply(2, 16, 2.0, e(), e(), p(), p(), p(), p(), p(F64), NULL, stream), EINVAL),
              ("bn_bwd_apply_fused sums=NULL", lib.omnipq_bn_bwd_apply_fused(2, 16, 2.0, e(), e(), p(), p(), p(), p(), NULL, e(), NULL,
                                                                             NULL, stream), EINVAL),
              ("sums_to_f32 dgamma=NULL", lib.omnipq_sums_to_f32(16, p(F64), p(), NULL, stream), EINVAL),
              ("gather idx=NULL", lib.omnipq_sa_gather(1, 5, 2, 2, 8, 16, 1.0, p(), p(), NULL, e(), e(), NULL, stream), EINVAL),
              ("scatter dxyz without dcentre", lib.omnipq_sa_scatter(1, 5, 2, 2, 8, 16, 1.0, p(I32), e(), p(), p(), NULL, stream), EINVAL),
              ("scatter_rows_csr no dfeat", lib.omnipq_sa_scatter_rows_csr(1, 5, 2, 2, 16, 1.0, p(I32), p(I32), e(), e(), NULL, 0, NULL,
                                                                           NULL, NULL, NULL, stream), EINVAL)]
    for count in (0.0, -1.0):
        table.append((f"pool_select_finalize count={count}",
                      lib.omnipq_sa_pool_select_finalize(2, 16, e(), e(), p(U8), p(U8), p(F64), count, p(), p(), 1e-5, 0.1, NULL, NULL,
                                                         p(), p(), p(), p(), p(), e(), p(U8), e(), NULL, stream), EINVAL))
    # nothing to do: OK, and nothing written
    # (no scene at all: with b > 0 and no ball the CSR forms still owe every point a zero, which is a write)
    table += [(f"{n} b=0", rc, OK) for n, rc in streaming_calls(16, b=0)]
    table += [(f"{n} rows=0", rc, OK) for n, rc in streaming_calls(16, rows=0, csr=False)]
    table += [("pool_bwd_apply_gb rows=0 gb=NULL", lib.omnipq_sa_pool_bwd_apply_gb(1, 0, 2, 16, 4.0, e(), p(), p(), p(), p(F64), p(), e(),
                                                                                   p(U8), e(), NULL, NULL, stream), EINVAL)]
    for name, rc, want in table:
        assert rc == want, (name, rc, want)
    assert ar.touched() == [], "a rejected or empty call wrote something"


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
def test_empty_batches_still_publish(dtype):
    """P = 0.  The statistics entries clear (or leave) the totals; the finalize entries publish a, b, mean, invstd; both apply
    entries that copy the totals publish dbeta | dgamma.  Nothing else is written.  count <= 0 in omnipq_bn_finalize /
    omnipq_bn_finalize_relu is accepted (include/omnipq_sa.h): OK; at count = 0 nothing they publish is finite."""
    lib, stream = lib_of(dtype)
    C = 16
    inp = sr.finalize_inputs(sr.by_id(sr.FINALIZE_CASES, "fin-C16"))
    ref = sr.finalize_reference(inp)
    # statistics over no rows
    for z, fn in ((False, lib.omnipq_colstats), (True, lib.omnipq_colstats_z)):
        sums, y = Buf(2 * C, F64, inp["sums"] if z else None), Buf(64, dtype)
        run(fn(0, C, P(y), P(sums), stream))
        assert y.blank() and torch.equal(sums.get(2, C), inp["sums"] if z else torch.zeros((2, C), dtype=F64))
    sums, junk = Buf(3 * C, F64), [Buf(64, dt) for dt in (dtype, dtype, F32, F32, F32, F32)]
    run(lib.omnipq_bn_bwd_stats(0, C, *[P(j) for j in junk], P(sums), stream))
    assert not bool(sums.get(3, C)[:2].any()) and _third_row_untouched(sums, C) and all(j.blank() for j in junk)
    # finalize with no rows to normalise / no balls to pool
    for entry in ("relu", "select"):
        fin = dict(inp, bias=None) if entry == "select" else inp
        got, extra = _finalize_call(lib, stream, fin, entry, dtype, y=torch.zeros((0, C) if entry == "relu" else (0, 3, C), dtype=dtype))
        report(dtype, f"empty-{entry}", got, sr.finalize_reference(fin))
        assert all(b.blank() for b in extra.values())
    assert ref[0]["a"].shape == (C,)
    # dbeta | dgamma from both apply entries
    totals = torch.arange(2 * C, dtype=F64).reshape(2, C) / 3.0 - 1.0
    sums, gbo, junk = Buf(3 * C, F64, totals), Buf(2 * C, F32), [Buf(64, dt) for dt in (dtype, F32, F32, F32, F32, dtype, U8, dtype)]
    Y, a, mean, invstd, g_out, out_pm, arg, dY = [P(j) for j in junk]
    run(lib.omnipq_sa_pool_bwd_apply_gb(1, 0, 4, C, 1.0, Y, a, mean, invstd, P(sums), g_out, out_pm, arg, dY, P(gbo), NULL, stream))
    assert torch.equal(sr.bits(gbo.get(2, C)), sr.bits(totals.to(F32))) and sums.unchanged() and all(j.blank() for j in junk)
    assert _third_row_untouched(sums, C)
    gbo = Buf(2 * C, F32)
    run(lib.omnipq_bn_bwd_apply_fused(0, C, 1.0, dY, Y, a, a, mean, invstd, P(sums), dY, P(gbo), NULL, stream))
    assert torch.equal(sr.bits(gbo.get(2, C)), sr.bits(totals.to(F32))) and sums.unchanged() and all(j.blank() for j in junk)
    # count <= 0: accepted.  count = 0 (an empty batch's own totals): 0 / 0, nothing published is finite
    for count in (0.0, -2.0):
        zero = dict(inp, cnt=count, sums=torch.zeros((2, C), dtype=F64), rm=None, rv=None)
        for entry in ("plain", "relu"):
            got, _ = _finalize_call(lib, stream, zero, entry, dtype, y=torch.zeros((0, C), dtype=dtype))
            assert count < 0 or not any(bool(torch.isfinite(got[n]).any()) for n in FIN_OUT), (entry, count)
