"""GPU: the NT and TN GEMMs (csrc/gemm_bf16.hip, csrc/gemm_tn_bf16.hip) through the C ABI against the float64 reference,
ELEMENT BY ELEMENT, on every route of the dispatcher.

omnipq_gemm_nt_e16 / _bias / _f32 / _stats / _ws / _splitk and omnipq_gemm_tn_e16 / _colsum are called directly, on the
library of the case's element type, on buffers this module lays out itself: every operand and every output lies in a flat
buffer filled with a NaN pattern, with 64 guard elements in front and behind and a 16-byte aligned base; operands are written
into their pitched views, so a read between the rows poisons the result.  After the call every element of C must be inside
the bound tests/gemm_reference.py derives for it (no exceptions, no norms), and every pad column, every guard and the
workspace's guards must still hold the pattern.  The cases are gemm_reference.CASES, natural shapes that reach every
production route without process-wide switches -- the CPU suite holds an emulation of the kernels' arithmetic, and seven
mutants of it, against the same bounds on the same cases (tests/test_gemm_reference.py).  The one-hot kind is exact: an e16
output must be bit-equal to the permuted entries of B, an f32 output equal; so is the small-integer kind of the f32 outputs,
whatever the order of summation.

Each test prints `RATIO <library> <case id>: C=<largest error / bound> ...` (pytest -s).
Measured on an MI355X (gfx950), the largest ratio per route and output over the route's cases, all 146 cases inside:

    route         output    bf16    f16        route                  cases take it through
    nt64-kres     e16      0.647   0.643       64 x 64 tiles, K <= 320 resident in LDS (_e16, _bias)
    nt64-stream   e16      0.640   0.566       64 x 64 tiles, streamed (_e16, _bias, _ws with a padded C)
    nt64-stream   f32      0.022   0.023       ... the f32 output (_f32: it has no K-resident variant)
    nt128         e16      0.663   0.662       128 x 128 tiles, 258 of them (_e16, _bias, _stats)
    nt128         f32      0.029   0.038       ... (_f32)
    nt128         sums     0.017   0.014       ... the statistics of _stats, partial-sum path
    ws-split64    e16      0.588   0.406       _ws split over 3 and 8 slabs of 64 x 64 tiles
    splitk        f32      0.008   0.007       _splitk, 1 to 3 slabs in use
    tn            f32      0.027   0.034       _tn_e16 / _tn_e16_colsum, 1 to 34 slabs
    tn            colsum   0.000   0.006

The e16 outputs sit at the single rounding on store (1 / MARGIN = 0.667 is a rounding error of exactly half a unit in the
last place); the CPU emulation (f32 accumulation in steps of 32, one rounding) stays at or below 0.66 on the same cases.
The split of 128 x 128 tiles inside omnipq_gemm_nt_e16_ws is not reachable from any entry point and has no case.
"""
import ctypes

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import gemm_reference as gr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                                    # elements in front of and behind every buffer
# a NaN of each type as the integer it is stored as
PATTERN = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC12345, torch.float64: 0x7FF8000012345678}
INT_OF = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def lib_of(dtype):
    import sa_fused
    ext = sa_fused._ext
    if dtype is torch.float16 and ext.LIB_F16_PATH is None:
        pytest.skip("no IEEE-half library in this build")
    return ext._LIBS[dtype], ext


class Buf:
    """rows x cols elements with row pitch ld inside a flat, pattern-filled buffer with guards on both sides"""

    def __init__(self, rows, cols, ld, dtype, value=None):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.flat = torch.empty(rows * ld + 2 * GUARD, dtype=dtype, device=DEV)
        self.flat.view(INT_OF[dtype]).fill_(PATTERN[dtype])
        assert (self.flat.data_ptr() + GUARD * self.flat.element_size()) % 16 == 0
        if value is not None:
            self.view().copy_(value.to(DEV) if isinstance(value, torch.Tensor) else torch.full((rows, cols), value, dtype=dtype))

    def view(self):
        return self.flat.as_strided((self.rows, self.cols), (self.ld, 1), GUARD)

    def ptr(self):
        return ctypes.c_void_p(self.flat.data_ptr() + GUARD * self.flat.element_size())

    def get(self):
        return self.view().cpu()

    def untouched(self, all_of_it=False):
        """every element outside the view (all_of_it: every element) still holds the pattern"""
        owned = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        if not all_of_it:
            owned.as_strided((self.rows, self.cols), (self.ld, 1), GUARD).fill_(True)
        return bool((self.flat.view(INT_OF[self.dtype])[~owned] == PATTERN[self.dtype]).all())


NULL = ctypes.c_void_p(0)


def run_case(case):
    """-> got {output: CPU tensor}, extras (the stored statistics, if any)"""
    lib, ext = lib_of(case["dtype"])
    e, M, N, K, dt = case["entry"], case["M"], case["N"], case["K"], case["dtype"]
    A, B, bias, ref, bnd = gr.case_data(case["id"])
    plan = gr.plan(case)
    stream = ext._stream(0)
    f32 = torch.float32
    a = Buf(A.shape[0], A.shape[1], case["lda"], dt, A)
    b = Buf(B.shape[0], B.shape[1], case["ldb"], dt, B)
    c = Buf(M, N, case["ldc"], f32 if gr.out_f32(case) else dt)
    bvec = Buf(1, N, N, f32, bias.reshape(1, N)) if bias is not None else None
    bias_p = bvec.ptr() if bvec is not None else NULL
    ws = Buf(1, max(plan["ws_floats"], 4), max(plan["ws_floats"], 4), f32)
    bufs, got, extra = [a, b, c, ws] + ([bvec] if bvec is not None else []), {}, {}
    if e == "e16":
        rc = lib.omnipq_gemm_nt_e16(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), c.ld, NULL, stream)
    elif e == "bias":
        rc = lib.omnipq_gemm_nt_e16_bias(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), c.ld, bias_p, stream)
    elif e == "f32":
        rc = lib.omnipq_gemm_nt_e16_f32(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), c.ld, stream)
    elif e == "ws":
        assert int(lib.omnipq_gemm_nt_workspace_floats(M, N, K)) == plan["ws_floats"] > 0
        rc = lib.omnipq_gemm_nt_e16_ws(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), c.ld, bias_p, ws.ptr(), stream)
    elif e == "splitk":
        assert c.ld == N
        rc = lib.omnipq_gemm_nt_e16_splitk(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), case["slabs"], ws.ptr(), stream)
    elif e == "stats":
        assert int(lib.omnipq_gemm_nt_stats_workspace_floats(M, N)) == plan["stats_ws_floats"] > 0
        sums = Buf(2, N, N, torch.float64, gr.SUMS_START)
        sws = Buf(1, plan["stats_ws_floats"], plan["stats_ws_floats"], f32)
        bufs += [sums, sws]
        rc = lib.omnipq_gemm_nt_e16_stats(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), c.ld, bias_p, sums.ptr(),
                                          sws.ptr(), NULL, stream)
        extra["sums"] = sums
    else:
        assert e in gr.TN_ENTRIES and c.ld == N
        assert int(lib.omnipq_gemm_tn_workspace_floats(M, N, K)) == plan["ws_floats"]
        if e == "tn":
            rc = lib.omnipq_gemm_tn_e16(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), ws.ptr(), NULL, stream)
        else:
            cs = Buf(1, M, M, f32, gr.COLSUM_START)
            bufs.append(cs)
            rc = lib.omnipq_gemm_tn_e16_colsum(M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), ws.ptr(), cs.ptr(), NULL, stream)
            extra["colsum"] = cs
    assert rc == 0, rc
    torch.cuda.synchronize()
    got["C"] = c.get()
    if "colsum" in extra:
        got["colsum"] = extra["colsum"].get().reshape(M)
    for buf in bufs:
        assert buf.untouched(), "wrote outside an output, or into an operand's pads"
    assert torch.equal(a.get().view(torch.int16), A.view(torch.int16)) and torch.equal(b.get().view(torch.int16),
                                                                                       B.view(torch.int16))
    if e == "ws" and plan["route"] != "ws-split64":
        assert ws.untouched(all_of_it=True), "a padded C must not split"
    return got, extra


def check(id):
    case = gr.case_of(id)
    got, extra = run_case(case)
    A, B, bias, ref, bnd = gr.case_data(id)
    rat = gr.ratios(got, ref, bnd)
    if "sums" in extra:                                 # the statistics against the float64 sums of what was STORED
        want, sbnd = gr.stats_reference(got["C"], torch.full((2, case["N"]), gr.SUMS_START, dtype=torch.float64))
        rat.update(gr.ratios(dict(sums=extra["sums"].get()), dict(sums=want), dict(sums=sbnd)))
    print(f"\n  RATIO {gr.lib_name(case['dtype'])} {id}: {gr.fmt(rat)}")
    assert set(rat) == {"C"} | set(extra)
    assert not gr.outside(rat), (id, gr.outside(rat))
    if case["kind"] in gr.EXACT_KINDS:
        assert all(torch.equal(got[n].double(), ref[n]) for n in got), "an exact kind is not exact"
    if case["kind"] == "onehot":
        want = gr.onehot_expected(case, B)
        if gr.out_f32(case):
            assert torch.equal(got["C"], want.float())
        else:
            assert torch.equal(got["C"].view(torch.int16), want.view(torch.int16))
        if "colsum" in got:                             # one position per channel (7 p) mod M, on top of what was there
            hit = torch.zeros(case["M"])
            hit[(7 * torch.arange(case["K"])) % case["M"]] = 1.0
            assert torch.equal(got["colsum"], hit + gr.COLSUM_START)


@pytest.mark.parametrize("id", gr.CASE_IDS)
def test_every_element_is_inside_its_bound(id):
    check(id)
