"""Float64 reference of the NT and TN GEMMs (csrc/gemm_bf16.hip, csrc/gemm_tn_bf16.hip), the elementwise error bounds their
arithmetic allows, a CPU emulation of that arithmetic with seven mutants, a restatement of the dispatcher's rules, and the
case table both suites walk (tests/test_gemm_reference.py on the CPU, tests/test_gpu_gemm_f64.py on the GPU).  Plain torch on
the CPU.

    NT   C[M][N] = A[M][K] B[N][K]^T (+ bias[n])        e16 or f32 output
    TN   C[M][N] = A[P][M]^T B[P][N]  (f32),  colsum[m] += sum_p A[p][m]  (f32 atomics, ADDED to what is there)

The reference is evaluated in float64 from the e16-ROUNDED operands (the tensors the kernels read).

Bounds, per element.  u = unit roundoff of the element type (2^-8 bfloat16, 2^-11 half), eta = 0 for bfloat16 (subnormals at
1e-38) and half's subnormal spacing 2^-24; S = |A| |B|^T (+ |bias|) resp. |A|^T |B| in float64; n = the contraction length.

    e16 output   MARGIN (u |ref| + n 2^-24 S) + eta      the single rounding on store + f32 accumulation
    f32 output   MARGIN n 2^-24 S
    colsum       MARGIN P 2^-24 (sum_p |A| + |initial|)
    sums         MARGIN STATS_DEPTH 2^-24 sum_m |y| resp. sum_m y^2, against the float64 sums of the STORED y (see below)

The product of two e16 values is exact in f32 for both types (8 + 8 resp. 11 + 11 significand bits), so the only errors are
those of the f32 additions, and n 2^-24 S bounds them for ANY order of summation: split-K, slab order and the MFMA's block
order need no model of their own.  MARGIN = 1.5 as in attention_reference.py, for what is not modelled; it is not tuned to
any result.

`sums` (omnipq_gemm_nt_e16_stats: column sums of y and y^2 over the stored e16 values y, f32 partial sums, f64 across them):
y and y^2 are exact in f32, and a value that passes through d f32 additions on its way into a sum carries at most
((1 + 2^-24)^d - 1) of its size as error.  In the kernel a stored value passes through at most 8 additions in its thread
(rows per thread of a 128 x 128 tile), 16 in the fold over the row groups and, on the partial-sum path, 22 in
partial_reduce_kernel (fewer than 128 row tiles per slab up to 8192 row tiles: 15 rounds over 8 accumulators and a tail of 7
into the first) before everything turns f64: STATS_DEPTH = 8 + 16 + 22 = 46 covers every route.
"""
import functools
import math

import torch

MARGIN = 1.5
STATS_DEPTH = 46
F32_EPS = 2.0 ** -24
GBK = 32                                # contraction elements per K-step, both kernels


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def abs_roundoff(dtype):
    return {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24}[dtype]


def lib_name(dtype):
    return {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]


# ---- reference and bounds ---------------------------------------------------------------------------------------------------

def reference_nt(A, B, bias=None):
    """-> dict(C, S), float64"""
    a, b = A.double(), B.double()
    C, S = a @ b.T, a.abs() @ b.abs().T
    if bias is not None:
        C, S = C + bias.double(), S + bias.double().abs()
    return dict(C=C, S=S, n=A.shape[1])


def reference_tn(A, B, colsum0=None):
    """A (P, M), B (P, N) -> dict(C, S, colsum, colabs), float64; colsum0: what the colsum buffer held before the call"""
    a, b = A.double(), B.double()
    out = dict(C=a.T @ b, S=a.abs().T @ b.abs(), n=A.shape[0])
    if colsum0 is not None:
        out["colsum"] = a.sum(dim=0) + colsum0.double()
        out["colabs"] = a.abs().sum(dim=0) + colsum0.double().abs()
    return out


def bounds(ref, dtype, out_f32):
    """-> {output: float64 bound per element} for C (and colsum, if the reference has one)"""
    n = ref["n"]
    acc = n * F32_EPS * ref["S"]
    if out_f32:
        b = dict(C=MARGIN * acc)
    else:
        b = dict(C=MARGIN * (unit_roundoff(dtype) * ref["C"].abs() + acc) + abs_roundoff(dtype))
    if "colsum" in ref:
        b["colsum"] = MARGIN * n * F32_EPS * ref["colabs"]
    return b


def stats_reference(C_stored, sums0):
    """what omnipq_gemm_nt_e16_stats adds to `sums` (double[2][N], sums0 before the call), from the STORED C, and its bound"""
    y = C_stored.double()
    want = torch.stack([y.sum(dim=0), (y * y).sum(dim=0)]) + sums0.double()
    bnd = MARGIN * STATS_DEPTH * F32_EPS * torch.stack([y.abs().sum(dim=0), (y * y).sum(dim=0)])
    return want, bnd


def ratios(got, ref, bnd):
    """got, ref, bnd: {output: tensor}.  -> {output: (largest error / bound, number of elements outside)}; an element that
    is not finite, or off where the bound is zero, counts as outside with ratio inf."""
    out = {}
    for name, g in got.items():
        err = (g.double() - ref[name]).abs()
        bd = bnd[name]
        assert err.shape == bd.shape, (name, err.shape, bd.shape)
        inside = err <= bd                               # NaN compares false
        r = err / bd
        r = torch.where((bd == 0) & (err == 0), torch.zeros_like(r), r)
        r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
        out[name] = (float(r.max()), int((~inside).sum()))
    return out


def outside(rat):
    return {n: r for n, r in rat.items() if r[1]}


def fmt(rat):
    return " ".join(f"{n}={r[0]:.3f}" for n, r in rat.items())


# ---- the dispatcher's rules, restated from include/omnipq_sa.h and the comments of the two sources -------------------------------

def cdiv(a, b):
    return (a + b - 1) // b


ROUTES = ("nt64-kres", "nt64-stream", "nt128", "ws-split64", "splitk", "tn")
TN_ENTRIES = ("tn", "tn_colsum")


def nt_small_tiles(M, N):
    """NT takes 64 x 64 tiles iff at most 256 tiles of 128 x 128 would be launched"""
    return cdiv(M, 128) * cdiv(N, 128) <= 256


def ws_split_slabs(M, N, K):
    """the slab count omnipq_gemm_nt_workspace_floats is sized for: 1 = no split.  Splits of 64 x 64 tiles only: the plan of
    128 x 128 tiles behind them is not reachable from any entry point (K >= 768 leaves at least 2 slabs on the 64 x 64 plan
    whenever tiles <= 128), and no case goes there."""
    tiles = cdiv(M, 128) * cdiv(N, 128)
    if K < 768 or tiles > 128:
        return 1
    slabs = min(1024 // (cdiv(M, 64) * cdiv(N, 64)), K // 256, 8)
    assert slabs >= 2, "the unreachable 128 x 128 split plan"
    return slabs


def stats_partial(M):
    """statistics go through per-tile partial sums (and a workspace) iff there are more than 64 row tiles: M > 8192"""
    return M > 8192


def tn_slabs(M, N, P):
    tiles = cdiv(M, 128) * cdiv(N, 128)
    return max(1, min(cdiv(512, tiles), cdiv(P, GBK * 6)))


def plan(case):
    """-> dict(route, k_chunk, used, ws_floats, stats_ws_floats, two_stage): what the library must do with `case`"""
    e, M, N, K = case["entry"], case["M"], case["N"], case["K"]
    p = dict(k_chunk=K, used=1, ws_floats=0, stats_ws_floats=0, two_stage=False, stats_partial=False)
    if e in TN_ENTRIES:                                  # K is the position count P
        slabs = tn_slabs(M, N, K)
        p["k_chunk"] = cdiv(cdiv(K, slabs), GBK) * GBK
        p["used"] = cdiv(K, p["k_chunk"])
        p["ws_floats"] = (slabs + 16) * M * N
        p["two_stage"] = p["used"] > 32
        p["route"] = "tn"
        return p
    if e == "splitk":                                    # always 128 x 128 tiles, f32 partials, ldc == N
        p["k_chunk"] = max(GBK, cdiv(K // GBK, case["slabs"]) * GBK)
        p["used"] = cdiv(K, p["k_chunk"])
        p["ws_floats"] = case["slabs"] * M * N
        p["route"] = "splitk"
        return p
    if e == "ws":
        slabs = ws_split_slabs(M, N, K)
        p["ws_floats"] = slabs * M * N if slabs > 1 else 0          # sized by shape alone; a padded C does not split
        if slabs > 1 and case["ldc"] == N:
            p["k_chunk"] = cdiv(K // GBK, slabs) * GBK
            p["used"] = cdiv(K, p["k_chunk"])
            p["route"] = "ws-split64"
            return p
    if e == "stats":
        p["stats_partial"] = stats_partial(M)
        p["stats_ws_floats"] = cdiv(M, 128) * 2 * N if p["stats_partial"] else 0
    if nt_small_tiles(M, N) and not p["stats_partial"]:
        # (the f32 output has no K-resident variant: its 64 x 64 tiles are streamed at every K)
        p["route"] = "nt64-kres" if K <= 320 and e != "f32" else "nt64-stream"
    else:
        p["route"] = "nt128"
    return p


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def make_inputs(case):
    """-> A, B (e16), bias (f32 or None).  NT: A (M, K), B (N, K); TN: A (P, M), B (P, N).
    randn    A ~ N(0, 1), B ~ N(0, 1) / sqrt(contraction length), bias ~ N(0, 1)
    onehot   NT: row m of A is one-hot at column (7 m) mod K; TN: position p of A is one-hot at channel (7 p) mod M, P <= M.
             The product is a permutation of B's entries: exact in every format.
    int      A and B hold integers in [-2, 2] (f32 outputs only): every product and every partial sum is an integer below
             2^24, exact in f32 in ANY order of summation -- one dropped, doubled or misplaced term of a long contraction,
             which the bound n 2^-24 S is far too wide to see, changes the result."""
    e, M, N, K, dt = case["entry"], case["M"], case["N"], case["K"], case["dtype"]
    gen = torch.Generator().manual_seed(5000 + CASE_IDS.index(case["id"]))
    tn = e in TN_ENTRIES
    a_shape, b_shape = ((K, M), (K, N)) if tn else ((M, K), (N, K))
    A = torch.randn(a_shape, generator=gen)
    B = torch.randn(b_shape, generator=gen) / math.sqrt(K)
    bias = torch.randn(N, generator=gen) if case["bias"] else None
    if case["kind"] == "onehot":
        assert bias is None
        rows = torch.arange(a_shape[0])
        if tn:
            assert K <= M
        A = torch.zeros(a_shape)
        A[rows, (7 * rows) % a_shape[1]] = 1.0
    elif case["kind"] == "int":
        assert bias is None and out_f32(case) and 4 * K < 2 ** 24
        A = torch.randint(-2, 3, a_shape, generator=gen).float()
        B = torch.randint(-2, 3, b_shape, generator=gen).float()
    else:
        assert case["kind"] == "randn", case["kind"]
    return A.to(dt), B.to(dt), bias


EXACT_KINDS = ("onehot", "int")                          # the float64 reference is the exact result, in the output's format too


def onehot_expected(case, B):
    """the exact product of the one-hot kind, in B's own element type"""
    M, N, K = case["M"], case["N"], case["K"]
    if case["entry"] in TN_ENTRIES:
        C = torch.zeros((M, N), dtype=B.dtype)
        p = torch.arange(K)
        C[(7 * p) % M] = B                               # P <= M and 7 is coprime to the M in use: one position per channel
        return C
    return B[:, (7 * torch.arange(M)) % K].T.contiguous()


# ---- the kernels' arithmetic on the CPU -------------------------------------------------------------------------------------

MUTANTS = ("drop_last_kstep", "bias_after_round", "round_partials", "truncate", "leak_row", "pitch_k", "swap_pieces")


def _truncate(x, dt):
    """f32 -> e16 towards zero"""
    r = x.to(dt)
    bits = r.view(torch.int16).to(torch.int32) & 0xFFFF
    over = r.float().abs() > x.abs()                     # rounded away from zero: one step back in magnitude
    bits = torch.where(over, bits - 1, bits)
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return bits.to(torch.int16).view(dt)


def emulate_nt(A, B, bias, out_f32, k_chunk=None, mutant=None, lda=None):
    """f32 accumulation per 32-wide K-step inside every slab of k_chunk, the slabs' partial sums added in f32 in slab order,
    then the bias, then ONE rounding to e16 (none for an f32 output).  mutant: one of MUTANTS, a defect the bounds must
    catch.  lda: the pitch of A in its buffer (the pitch_k mutant reads that buffer with pitch K)."""
    assert mutant is None or mutant in MUTANTS
    dt = A.dtype
    M, K = A.shape
    N = B.shape[0]
    f32 = torch.float32
    a, b = A.to(f32), B.to(f32)
    if mutant == "pitch_k":
        assert lda is not None and lda > K
        flat = torch.zeros(M * lda, dtype=f32)
        flat.as_strided((M, K), (lda, 1)).copy_(a)
        a = flat[:M * K].reshape(M, K)
    k_chunk = K if k_chunk is None else k_chunk
    kend = K - GBK if mutant == "drop_last_kstep" else K
    total = torch.zeros((M, N), dtype=f32)
    for k0 in range(0, K, k_chunk):
        acc = torch.zeros((M, N), dtype=f32)
        for k in range(k0, min(k0 + k_chunk, kend), GBK):
            acc = acc + a[:, k:k + GBK] @ b[:, k:k + GBK].T
        if mutant == "round_partials":
            acc = acc.to(dt).to(f32)
        total = acc if k0 == 0 else total + acc
    if mutant == "leak_row":                             # a row past M (here: the values of row 0) in the last stored row
        total[M - 1] = total[M - 1] + 2.0 ** -7 * total[0 if M > 1 else M - 1]
    if bias is not None and mutant != "bias_after_round":
        total = total + bias.to(f32)
    if out_f32:
        C = total
    else:
        C = _truncate(total, dt) if mutant == "truncate" else total.to(dt)
        if bias is not None and mutant == "bias_after_round":
            C = (C.to(f32) + bias.to(f32)).to(dt)
    if mutant == "swap_pieces":
        assert N >= 16
        C = C.clone()
        C[:, 0:8], C[:, 8:16] = C[:, 8:16].clone(), C[:, 0:8].clone()
    return C


def emulate_tn(A, B, k_chunk, two_stage, colsum0=None):
    """f32 accumulation per step of 32 positions inside every slab, the slabs summed in f32 (through 16 groups when there
    are more than 32); colsum: one f32 sum per slab, added to what is there.  -> C, colsum (or None)"""
    f32 = torch.float32
    a, b = A.to(f32), B.to(f32)
    P = a.shape[0]
    parts, cs = [], None if colsum0 is None else colsum0.to(f32).clone()
    for p0 in range(0, P, k_chunk):
        acc = torch.zeros((a.shape[1], b.shape[1]), dtype=f32)
        col = torch.zeros(a.shape[1], dtype=f32)
        for p in range(p0, min(p0 + k_chunk, P), GBK):
            acc = acc + a[p:p + GBK].T @ b[p:p + GBK]
            col = col + a[p:p + GBK].sum(dim=0)
        parts.append(acc)
        if cs is not None:
            cs = cs + col
    if two_stage:
        parts = [functools.reduce(torch.add, parts[g::16]) for g in range(16)]
    return functools.reduce(torch.add, parts), cs


def emulate(case, A, B, bias, colsum0=None, mutant=None):
    """the case's entry point on the CPU -> {output: tensor}"""
    p = plan(case)
    if case["entry"] in TN_ENTRIES:
        assert mutant is None
        C, cs = emulate_tn(A, B, p["k_chunk"], p["two_stage"], colsum0 if case["entry"] == "tn_colsum" else None)
        return dict(C=C) if cs is None else dict(C=C, colsum=cs)
    return dict(C=emulate_nt(A, B, bias, out_f32(case), p["k_chunk"], mutant, case["lda"]))


def out_f32(case):
    return case["entry"] in ("f32", "splitk") + TN_ENTRIES


# ---- the cases --------------------------------------------------------------------------------------------------------------
# dict(id, entry, M, N, K, lda, ldb, ldc, dtype, kind, bias, slabs, route).  entry: e16 / bias / f32 / stats / ws / splitk are
# omnipq_gemm_nt_e16<_entry> (bias: with its bias; ws: with or without), tn / tn_colsum omnipq_gemm_tn_e16<_colsum> with
# K = the position count P, lda >= M and ldb >= N the pitches of A (P, M) and B (P, N), ldc == N.  route: what the
# dispatcher must do with it, written down here and checked against plan() and the library's workspace functions.
# These are the smallest shapes at which each route can still go wrong; the largest float64 reference is 16400 x 136 x 96.

def _cases():
    cs = []

    def add(entry, M, N, K, route, pad=False, kind="randn", bias=None, slabs=0, ldc=None, tag=""):
        tn = entry in TN_ENTRIES
        f32c = entry in ("f32",)
        bias = entry == "bias" if bias is None else bias
        if tn:
            lda, ldb, ldc_ = (M + 8, N + 16, N) if pad else (M, N, N)
        else:
            lda, ldb = (K + 8, K + 24) if pad else (K, K)
            # a padded C: N + 8 (N + 4 for the f32 output); the split entry points require ldc == N
            ldc_ = N if (not pad or entry == "splitk" or route == "ws-split64") else N + (4 if f32c else 8)
        if ldc is not None:
            ldc_ = ldc
        name = entry + ("+bias" if bias and entry != "bias" else "") + (f"-s{slabs}" if slabs else "")
        kinds = {"randn": "", "onehot": "-onehot", "int": "-int"}
        for dt in (torch.bfloat16, torch.float16):
            id = f"{lib_name(dt)}-{name}-{M}x{N}x{K}" + ("-pad" if pad else "") + kinds[kind] + tag
            cs.append(dict(id=id, entry=entry, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc_, dtype=dt, kind=kind, bias=bias,
                           slabs=slabs, route=route))

    # 64 x 64 tiles, K-resident (K <= 320 = ten K-steps); the f32 output streams its 64 x 64 tiles at every K
    for M, N, K in ((1, 8, 32), (72, 40, 32), (130, 72, 320)):
        add("e16", M, N, K, "nt64-kres")
        add("bias", M, N, K, "nt64-kres")
        add("f32", M, N, K, "nt64-stream")
    add("f32", 72, 12, 32, "nt64-stream")                # N % 8 != 0
    add("e16", 130, 72, 320, "nt64-kres", pad=True)
    add("bias", 130, 72, 320, "nt64-kres", pad=True)
    add("f32", 130, 72, 320, "nt64-stream", pad=True)
    add("f32", 72, 12, 32, "nt64-stream", pad=True)
    add("e16", 130, 72, 320, "nt64-kres", pad=True, kind="onehot")
    add("f32", 130, 72, 320, "nt64-stream", pad=True, kind="onehot")
    # 64 x 64 tiles, streamed: the first K that is not resident; eleven and seventeen steps
    for M, N, K in ((130, 72, 352), (77, 16, 544)):
        add("e16", M, N, K, "nt64-stream")
        add("bias", M, N, K, "nt64-stream")
    add("e16", 130, 72, 352, "nt64-stream", pad=True)
    add("bias", 130, 72, 352, "nt64-stream", pad=True)
    add("e16", 130, 72, 352, "nt64-stream", pad=True, kind="onehot")
    # 128 x 128 tiles at their natural size (258 tiles): the last M-tile holds 16 rows, the last N-tile 8 columns, the
    # statistics take the partial-sum path
    for entry in ("e16", "bias", "f32", "stats"):
        add(entry, 16400, 136, 96, "nt128")
        add(entry, 16400, 136, 96, "nt128", pad=True)
        add(entry, 33000, 8, 32, "nt128")
    add("stats", 16400, 136, 96, "nt128", bias=True)
    add("f32", 33000, 12, 32, "nt128")
    add("e16", 16400, 136, 96, "nt128", pad=True, kind="onehot")
    add("f32", 16400, 136, 96, "nt128", pad=True, kind="onehot")
    add("f32", 33000, 12, 32, "nt128", kind="int")
    # omnipq_gemm_nt_e16_ws: 3 slabs of 288 / 288 / 224; 8 slabs of 256; a padded C must NOT split (streamed, 25 steps)
    for bias in (False, True):
        add("ws", 72, 40, 800, "ws-split64", bias=bias)
        add("ws", 300, 96, 2048, "ws-split64", bias=bias)
        add("ws", 72, 40, 800, "nt64-stream", bias=bias, ldc=48, tag="-ldc48")
    add("ws", 72, 40, 800, "ws-split64", pad=True, bias=True)
    add("ws", 72, 40, 800, "ws-split64", pad=True, kind="onehot")
    # omnipq_gemm_nt_e16_splitk: one slab; 64 + 32; more slabs than K-steps; three slabs over two tiles
    for slabs in (1, 2, 5):
        add("splitk", 72, 44, 96, "splitk", slabs=slabs)
    add("splitk", 200, 136, 96, "splitk", slabs=3)
    add("splitk", 72, 44, 96, "splitk", slabs=2, pad=True)
    add("splitk", 72, 44, 96, "splitk", slabs=2, pad=True, kind="onehot")
    add("splitk", 72, 44, 96, "splitk", slabs=5, kind="int")
    add("splitk", 200, 136, 96, "splitk", slabs=3, kind="int")
    # TN (M, N, P): less than one step; one full tile; two slabs with a ragged second; 34 slabs (the two-stage slab
    # reduction); edge tiles on both axes
    for P, M, N in ((31, 8, 8), (32, 128, 128), (193, 72, 40), (6401, 8, 8), (1000, 136, 264)):
        add("tn", M, N, P, "tn")
        add("tn_colsum", M, N, P, "tn")
    add("tn", 72, 40, 193, "tn", pad=True)
    add("tn_colsum", 72, 40, 193, "tn", pad=True)
    add("tn_colsum", 128, 128, 32, "tn", pad=True, kind="onehot")
    for P, M, N, pad in ((31, 8, 8, False), (193, 72, 40, True), (6401, 8, 8, False), (1000, 136, 264, False)):
        add("tn_colsum", M, N, P, "tn", pad=pad, kind="int")
    return cs


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
COLSUM_START = 1.0                                       # what the colsum buffer holds before the call
SUMS_START = 1.0                                         # ... and the statistics buffer


def case_of(id):
    return CASES[CASE_IDS.index(id)]


@functools.lru_cache(maxsize=None)
def case_data(id):
    """-> A, B, bias, float64 reference, bounds of the case (computed once, shared, not to be modified)"""
    case = case_of(id)
    A, B, bias = make_inputs(case)
    if case["entry"] in TN_ENTRIES:
        cs0 = torch.full((case["M"],), COLSUM_START) if case["entry"] == "tn_colsum" else None
        ref = reference_tn(A, B, cs0)
    else:
        ref = reference_nt(A, B, bias)
    return A, B, bias, ref, bounds(ref, case["dtype"], out_f32(case))
