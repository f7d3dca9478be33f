"""Float64 reference of the decoder's row kernels (csrc/decoder_ops.hip), the elementwise error bounds their roundings
allow, an independent restatement of their dropout mask, a CPU emulation of the kernels' arithmetic, and the case tables
both suites walk.  Plain torch / numpy on the CPU.

The reference is evaluated in float64 from the tensors the kernels read: x, gamma, beta, g32 in f32; y, pe, g16, g16_pe
in e16 (the library's 16-bit type); p and eps as the f32 numbers the C ABI carries.  keep is the mask below.

    forward    r = x + keep y / (1 - p),  mu = mean_c r,  var = mean_c (r - mu)^2,  rstd = (var + eps)^-1/2
               xh = (r - mu) rstd,  out = xh gamma + beta,  out_pe = out + pe
    backward   t = g32 + g16 + g16_pe,  dgamma = sum_rows t xh,  dbeta = sum_rows t,  go = t gamma
               dx = rstd (go - mean_c go - xh mean_c (go xh)),  dy = keep dx / (1 - p)

The mask (`keep_mask`).  seed32 = dec_seed(seed word, salt), keep element i iff dec_hash(i, seed32) >= thresh with
thresh = clamp(floor(p 2^32), 1, 2^32 - 1) for p > 0 (p = 0: no mask at all) and i = row C + c -- csrc/common.h and
drop_params() of decoder_ops.hip restated in integer numpy.  The GPU suite takes its mask from here, never from a kernel.

Bounds (`bounds`).  u32 = 2^-24 per f32 operation; u = 2^-8 (bfloat16) or 2^-11 (half) per e16 store, eta = an absolute
term per e16 store (half's subnormal spacing 2^-24; bfloat16's 2^-133).  A row of C channels is summed as: 4 elements of a
chunk pairwise (2 additions deep), a lane's chunks in turn (ceil(C / 256)), a 6-step butterfly, times 1 / C -- D = 9 +
ceil(C / 256) roundings on the longest path.  |.| is elementwise, mean / sum run over a row's channels.  To first order:

    r       e_r   = u32 (|r| + 3 |keep y / (1 - p)|)                 1 / (1 - p) in f32, the product, the sum; 0 without y
    mu      e_mu  = u32 (D mean|r| + |mu|) + mean e_r                scales with mean|r|, not with |mu|
    r - mu  e_d   = e_mu + e_r + u32 |r - mu|
    var     e_var = mean(2 |d| (e_r + u32 |d|)) + mean(e_d^2) + (D + 2) u32 var
                    the common shift e_mu of every d enters var only in second order (sum d = 0): two-pass variance;
                    the second-order term is what is left of a constant row
    rstd    e_rs  = rstd (e_var + u32 (var + eps)) / (2 (var + eps)) + 2 u32 rstd        hardware rsqrt: 1 ulp
    xh      e_xh  = e_d rstd + |d| e_rs + u32 |xh|                   i.e. u32 (|r| + |mu|) rstd and up
    out     e_out = |gamma| e_xh + u32 (|xh gamma| + |out|);  out16: + u |out| + eta;  out_pe: + (u32 + u) |out_pe| + eta
    t       e_t   = (gradients given - 1) u32 sum_i |g_i|
    go      e_go  = |gamma| e_t + u32 |go|
    m1      e_m1  = mean e_go + D u32 mean|go|
    m2      e_m2  = mean(e_go |xh| + |go| e_xh + u32 |go xh|) + D u32 mean|go xh|      the backward inherits e_xh here
    dx      e_dx  = rstd (e_go + e_m1 + |xh| e_m2 + |m2| e_xh + u32 (|go - m1| + |xh m2| + |go - m1 - xh m2|))
                    + |go - m1 - xh m2| e_rs + u32 |dx|
    dy      keep (e_dx / (1 - p) + 3 u32 |dy|) + u |dy| + eta
    dgamma  sum_rows (e_t |xh| + |t| e_xh + u32 |t xh|) + n u32 (sum_rows |t xh| + |accumulator before|)
    dbeta   sum_rows e_t + n u32 (sum_rows |t| + |accumulator before|)
            n = the f32 additions on the longest path: rows one wave visits (ceil(R / (4 blocks))) + 3 to fold the block's
            four waves + one atomic per block (`blocks`; 0 on the partials route, whose rows the test sums in float64)

and all of it times MARGIN = 1.5 for what is not modelled (second-order terms, fused multiply-adds that skip a rounding
counted here, denormal results).  1.5 is the constant of attention_reference.py and gemm_reference.py; the derivation above
is a worst case per rounding, so nothing here argues for another one.

    omnipq_layernorm_param_reduce   out = out0 + sum_b part[b]: (blocks // 16 + 8) u32 (sum_b |part[b]| + |out0|)
                                    (a quarter's unrolled chain, its tail of at most 3, two pairwise folds, the atomic)
    relu + dropout and its backward zero exactly where dropped / gated; elsewhere (3 u32 + u) |value| + eta
    add_to_e16, add_n, merge_rows with g_joint     u |sum| + eta + (n - 1) u32 sum|terms|   (f32 add_n: no u, no eta)
    pad_rows, split_rows, merge_rows without g_joint, pad columns   bit equality (pad_rows from f32: one e16 rounding,
                                    the same rounding torch does)
"""
import math

import numpy as np
import torch

MARGIN = 1.5
U32 = 2.0 ** -24
LN_OUTPUTS = ("mean", "rstd", "out32", "out16", "out_pe", "dx", "dy", "dgb")
SEED, SALT = 0x1234567887654321, 5
EPS = 1e-5
F32 = torch.float32


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def abs_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}[dtype]


def as_f32(v):
    """the double a C float argument holds"""
    return float(np.float32(v))


# ---- the mask, restated -------------------------------------------------------------------------------------------------

def dec_seed(seed, salt):
    m64 = (1 << 64) - 1
    s = ((int(seed) & m64) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * ((int(salt) + 1) & 0xFFFFFFFF)) & m64
    return ((s >> 32) ^ s) & 0xFFFFFFFF


def dec_hash(idx, seed32):
    """idx: uint32 numpy array -> uint32 numpy array"""
    x = idx.astype(np.uint32) ^ np.uint32(seed32)
    x = x * np.uint32(0x9E3779B1)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x85EBCA77)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE3D)
    x = x ^ (x >> np.uint32(16))
    return x


def threshold(p):
    """0 = no dropout; else clamp(floor(p 2^32), 1, 2^32 - 1) of the f32 number p"""
    p = as_f32(p)
    assert 0.0 <= p < 1.0
    if p == 0.0:
        return 0
    return int(min(max(math.floor(p * 4294967296.0), 1), 4294967295))


def keep_mask(seed, salt, p, rows, cols, pitch=None):
    """-> bool (rows, cols): element (row, c) has index row * pitch + c (pitch = cols unless a defect is being modelled)"""
    th = threshold(p)
    if th == 0:
        return torch.ones((rows, cols), dtype=torch.bool)
    pitch = cols if pitch is None else pitch
    idx = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(pitch) + np.arange(cols, dtype=np.uint64)[None, :])
    h = dec_hash((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), dec_seed(seed, salt))
    return torch.from_numpy(h >= np.uint32(th))


# ---- ratios -------------------------------------------------------------------------------------------------------------

def ratios(got, want, bnd):
    """got, want, bnd: {output: tensor}.  -> {output: (largest error / bound, number of elements outside)} over got's keys;
    an element that is not finite, or off where the bound is zero, counts as outside with ratio inf."""
    out = {}
    for name, g in got.items():
        err = (g.double() - want[name].double()).abs()
        bd = bnd[name]
        assert err.shape == bd.shape, (name, err.shape, bd.shape)
        inside = err <= bd                               # NaN compares false
        r = err / bd
        r = torch.where((bd == 0) & (err == 0), torch.zeros_like(r), r)
        r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
        out[name] = (float(r.max()) if r.numel() else 0.0, int((~inside).sum()))
    return out


def outside(rat):
    return {n: r for n, r in rat.items() if r[1]}


def fmt(rat):
    return " ".join(f"{n}={r[0]:.3f}" for n, r in rat.items())


# ---- LayerNorm: reference and bounds ------------------------------------------------------------------------------------

def ln_blocks(R):
    """workgroups of the backward (omnipq_add_dropout_layernorm_bwd_blocks, restated)"""
    return min((R + 3) // 4, 512)


def reference(inp, keep, p, eps=EPS):
    """inp: dict(x, y|None, gamma, beta, pe|None, g32|None, g16|None, gpe|None, acc0 (2C) | None).  -> dict of float64"""
    p, eps = as_f32(p), as_f32(eps)
    x = inp["x"].double()
    gamma, beta = inp["gamma"].double(), inp["beta"].double()
    yk = torch.zeros_like(x) if inp["y"] is None else keep.double() * inp["y"].double() / (1.0 - p)
    r = x + yk
    mu = r.mean(dim=1, keepdim=True)
    d = r - mu
    var = (d * d).mean(dim=1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xh = d * rstd
    out = xh * gamma + beta
    ref = dict(r=r, yk=yk, mu=mu, var=var, xh=xh, d=d, gamma=gamma, eps=eps, p=p, has_y=inp["y"] is not None,
               keep=keep.double(), mean=mu.squeeze(1), out32=out, out16=out, rstd_col=rstd)
    ref["rstd"] = rstd.squeeze(1)                       # as the kernel stores it; rstd_col broadcasts over a row
    if inp["pe"] is not None:
        ref["out_pe"] = out + inp["pe"].double()
    gs = [inp[n].double() for n in ("g32", "g16", "gpe") if inp[n] is not None]
    t = sum(gs) if gs else torch.zeros_like(x)
    go = t * gamma
    m1 = go.mean(dim=1, keepdim=True)
    m2 = (go * xh).mean(dim=1, keepdim=True)
    inner = go - m1 - xh * m2
    dx = rstd * inner
    acc0 = torch.zeros(2 * x.shape[1], dtype=torch.float64) if inp.get("acc0") is None else inp["acc0"].double()
    ref.update(gs=gs, t=t, go=go, m1=m1, m2=m2, inner=inner, dx=dx, acc0=acc0,
               dgb=acc0 + torch.cat([(t * xh).sum(dim=0), t.sum(dim=0)]))
    if ref["has_y"]:
        ref["dy"] = keep.double() * dx / (1.0 - p)
    return ref


def bounds(ref, dtype, route="atomic"):
    """-> {output: float64 bound per element}; route: "atomic" (dgb is the accumulator) or "partials" (dgb is the float64
    sum of the partial rows)"""
    u, eta = unit_roundoff(dtype), abs_roundoff(dtype)
    r, mu, d, var, xh, gamma = ref["r"], ref["mu"], ref["d"], ref["var"], ref["xh"], ref["gamma"].abs()
    rstd = ref["rstd_col"]
    R, C = r.shape
    D = 9 + (C + 255) // 256

    def mean(v):
        return v.mean(dim=1, keepdim=True)

    e_r = U32 * (r.abs() + 3.0 * ref["yk"].abs()) if ref["has_y"] else torch.zeros_like(r)
    e_mu = U32 * (D * mean(r.abs()) + mu.abs()) + mean(e_r)
    e_d = e_mu + e_r + U32 * d.abs()
    e_var = mean(2.0 * d.abs() * (e_r + U32 * d.abs())) + mean(e_d * e_d) + (D + 2) * U32 * var
    ve = var + ref["eps"]
    e_rs = rstd * (e_var + U32 * ve) / (2.0 * ve) + 2.0 * U32 * rstd
    e_xh = e_d * rstd + d.abs() * e_rs + U32 * xh.abs()
    out = ref["out32"]
    e_out = gamma * e_xh + U32 * ((xh * gamma).abs() + out.abs())
    b = dict(mean=e_mu.squeeze(1), rstd=e_rs.squeeze(1), out32=e_out, out16=e_out + u * out.abs() + eta)
    if "out_pe" in ref:
        b["out_pe"] = e_out + (U32 + u) * ref["out_pe"].abs() + eta
    gs, t, go, m1, m2, inner, dx = (ref[n] for n in ("gs", "t", "go", "m1", "m2", "inner", "dx"))
    e_t = (len(gs) - 1) * U32 * sum(g.abs() for g in gs) if len(gs) > 1 else torch.zeros_like(r)
    e_go = gamma * e_t + U32 * go.abs()
    e_m1 = mean(e_go) + D * U32 * mean(go.abs())
    gx = go * xh
    e_m2 = mean(e_go * xh.abs() + go.abs() * e_xh + U32 * gx.abs()) + D * U32 * mean(gx.abs())
    e_in = e_go + e_m1 + xh.abs() * e_m2 + m2.abs() * e_xh + U32 * ((go - m1).abs() + (xh * m2).abs() + inner.abs())
    e_dx = rstd * e_in + inner.abs() * e_rs + U32 * dx.abs()
    b["dx"] = e_dx
    if ref["has_y"]:
        dy = ref["dy"]
        b["dy"] = ref["keep"] * (e_dx / (1.0 - ref["p"]) + 3.0 * U32 * dy.abs()) + u * dy.abs() + eta
    blocks = ln_blocks(R)
    n = -(-R // (4 * blocks)) + 3 + (blocks if route == "atomic" else 0)
    tx = t * xh
    e_tx = e_t * xh.abs() + t.abs() * e_xh + U32 * tx.abs()
    acc0 = ref["acc0"].abs()
    b["dgb"] = torch.cat([e_tx.sum(dim=0) + n * U32 * (tx.abs().sum(dim=0) + acc0[:C]),
                          e_t.sum(dim=0) + n * U32 * (t.abs().sum(dim=0) + acc0[C:])])
    return {k: MARGIN * v for k, v in b.items()}


# ---- LayerNorm: the kernels' arithmetic in f32 ----------------------------------------------------------------------------

MUTANTS = ("one_pass_var", "padded_divisor", "eps_after_sqrt", "no_m2", "dy_no_scale", "mask_padded_pitch",
           "dgb_drop_tail_rows", "pe_double_rounding", "bwd_g32_only", "reduce_no_tail", "relu_gate_from_grad")
_LANE = torch.arange(64)


def _wave_sum(v):
    """(R, 64) -> (R,): the xor butterfly of wave_sum(), every lane ends with the same bits"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, _LANE ^ o]
    return v[:, 0]


def _lanes(x):
    """(R, C) -> (R, 4, 64, 4): [row, chunk slot i, lane, element] -- chunk lane + 64 i of the row, zeros past C"""
    R, C = x.shape
    return torch.cat([x, torch.zeros((R, 1024 - C), dtype=x.dtype)], dim=1).reshape(R, 4, 64, 4)


def _lane_sum(v, C):
    """sum over a row of per-element values the way a lane accumulates them: chunk by chunk, element by element"""
    L, acc = _lanes(v), torch.zeros((v.shape[0], 64), dtype=F32)
    valid = (torch.arange(4)[:, None] * 64 + _LANE[None, :]) < C // 4
    for i in range(4):
        for e in range(4):
            acc = torch.where(valid[i], acc + L[:, i, :, e], acc)
    return _wave_sum(acc)


def keep_inv_f32(p):
    one = torch.tensor(1.0, dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


def rnd(x, dtype):
    return x.to(dtype).to(F32)


def emulate(inp, keep, p, dtype, eps=EPS, mutant=None, seed=SEED, salt=SALT):
    """f32 arithmetic in the kernels' order: a lane's chunk sums, the butterfly, two-pass variance, rsqrt, the e16 stores,
    the backward's per-wave accumulators, the fold of a block's four waves and one addition per block for the atomics.
    -> {output: tensor}: every LN_OUTPUTS entry the inputs ask for, plus "part" (blocks, 2C), the partials route."""
    assert mutant is None or mutant in MUTANTS
    x, y, gamma, beta, pe = (inp[n] for n in ("x", "y", "gamma", "beta", "pe"))
    R, C = x.shape
    ki = keep_inv_f32(p)
    drop = y is not None and threshold(p) > 0
    if mutant == "mask_padded_pitch" and drop:
        keep = keep_mask(seed, salt, p, R, C, pitch=256 * ((C + 255) // 256))
    zero = torch.zeros((), dtype=F32)
    r = x.clone()
    if y is not None:
        v = y.to(F32)
        r = x + (torch.where(keep, v * ki, zero) if drop else v)
    invC = torch.tensor(1.0, dtype=F32) / torch.tensor(float(256 * ((C + 255) // 256) if mutant == "padded_divisor" else C),
                                                       dtype=F32)
    L = _lanes(r)
    s = torch.zeros((R, 64), dtype=F32)
    for i in range(4):
        s = s + ((L[:, i, :, 0] + L[:, i, :, 1]) + (L[:, i, :, 2] + L[:, i, :, 3]))
    mu = (_wave_sum(s) * invC)[:, None]
    if mutant == "one_pass_var":
        var = (_lane_sum(r * r, C) * invC)[:, None] - mu * mu
    else:
        d = r - mu
        var = (_lane_sum(d * d, C) * invC)[:, None]
    eps32 = torch.tensor(eps, dtype=F32)
    rs = 1.0 / (torch.sqrt(var) + eps32) if mutant == "eps_after_sqrt" else torch.rsqrt(var + eps32)
    out = (r - mu) * rs * gamma + beta
    got = dict(mean=mu.squeeze(1), rstd=rs.squeeze(1), out32=out, out16=out.to(dtype))
    if pe is not None:
        got["out_pe"] = ((rnd(out, dtype) if mutant == "pe_double_rounding" else out) + pe.to(F32)).to(dtype)
    # backward
    xh = (r - mu) * rs
    t = torch.zeros((R, C), dtype=F32)
    if inp["g32"] is not None:
        t = inp["g32"].clone()
    if inp["g16"] is not None and not (mutant == "bwd_g32_only" and inp["g32"] is not None):
        t = t + inp["g16"].to(F32)
    if inp["gpe"] is not None and not (mutant == "bwd_g32_only" and inp["g32"] is not None):
        t = t + inp["gpe"].to(F32)
    go = t * gamma
    m1 = (_lane_sum(go, C) * invC)[:, None]
    m2 = (_lane_sum(go * xh, C) * invC)[:, None]
    dx = rs * ((go - m1) if mutant == "no_m2" else (go - m1 - xh * m2))
    got["dx"] = dx
    if y is not None:
        if drop:
            got["dy"] = torch.where(keep, dx if mutant == "dy_no_scale" else dx * ki, zero).to(dtype)
        else:
            got["dy"] = dx.to(dtype)
    blocks = ln_blocks(R)
    K = -(-R // (4 * blocks))
    tt = t.clone()
    if mutant == "dgb_drop_tail_rows" and R % 4:
        tt[R - R % 4:] = 0.0
    both = torch.cat([tt * xh, tt], dim=1)                                  # (R, 2C): dgamma | dbeta terms
    both = torch.cat([both, torch.zeros((K * 4 * blocks - R, 2 * C), dtype=F32)]).reshape(K, blocks, 4, 2 * C)
    acc = torch.zeros((blocks, 4, 2 * C), dtype=F32)
    for k in range(K):
        acc = acc + both[k]
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    dgb = torch.zeros(2 * C, dtype=F32) if inp.get("acc0") is None else inp["acc0"].clone()
    for b in range(blocks):
        dgb = dgb + part[b]
    got.update(part=part, dgb=dgb)
    return got


def ln_ratios(got, ref, bnd):
    return ratios({n: got[n] for n in LN_OUTPUTS if n in got}, ref, bnd)


# ---- LayerNorm: inputs and cases ------------------------------------------------------------------------------------------
# kind    randn      x, y ~ N(0, 1)
#         offset     row mean ~1e3 (|mu| / sigma > OFFSET_RATIO), sigma ~1: a one-pass variance loses every digit
#         tiny       sigma ~1e-3 around zero: var ~1e-6 next to eps = 1e-5
#         constant   every channel of a row equal (y too): var = 0 exactly, rstd = eps^-1/2
#         mixed      one channel per row at 300, the others N(0, 1)
# gamma   plain      1 + 0.3 N(0, 1);   signed: N(0, 1) with every third entry 0
# outs    which of out32 / out16 / (pe, out_pe) are given: "32", "16", "both", "pe" (= both + pe)
# grads   which of g32 / g16 / g16_pe are given: "g32", "g16", "gpe", "all", "none"
# route   "atomic" (dgamma|dbeta added to a pre-filled accumulator) or "partials"
OFFSET_RATIO = 300.0
KINDS = ("randn", "offset", "tiny", "constant", "mixed")


def _case(id, R=5, C=260, kind="randn", gamma="plain", y=True, p=0.1, outs="pe", grads="all", route="atomic"):
    return dict(id=id, R=R, C=C, kind=kind, gamma=gamma, y=y, p=p, outs=outs, grads=grads, route=route)


def _cases():
    cs = []
    for C in (4, 8, 252, 256, 260, 288, 512, 516, 768, 772, 1020, 1024):       # a lane's 1st .. 4th chunk, full and one over
        cs.append(_case(f"C-{C}", C=C))
    for R in (1, 3, 4, 5, 37):                                                  # waves without a row, R % 4, ten blocks
        cs.append(_case(f"R-{R}", R=R, route="partials"))
    cs.append(_case("stride-fwd", R=8192 + 5, C=8))                             # forward: 2048 blocks x 4 waves, then 5 more
    cs.append(_case("stride-bwd", R=2048 + 5, C=260))                           # backward: 512 blocks x 4 waves, then 5 more
    cs.append(_case("stride-bwd-partials", R=2048 + 5, C=260, route="partials"))
    for kind in KINDS:
        cs.append(_case(f"kind-{kind}", R=37, C=288, kind=kind, p=0.0 if kind == "constant" else 0.1))
    cs.append(_case("kind-constant-noy", R=37, C=288, kind="constant", y=False, outs="both", grads="g32"))
    cs.append(_case("kind-offset-1024", C=1024, kind="offset"))
    cs.append(_case("gamma-signed", R=37, C=288, gamma="signed"))
    cs.append(_case("y-null", y=False, route="partials"))
    cs.append(_case("y-null-pe", R=37, C=288, y=False))
    for p in (0.0, 0.1, 0.5, 1e-12, 0.9):
        cs.append(_case(f"p-{p}", R=37, C=288, p=p))
    for outs in ("32", "16", "both", "pe"):
        cs.append(_case(f"outs-{outs}", outs=outs))
    for grads in ("g32", "g16", "gpe", "all", "none"):
        cs.append(_case(f"grads-{grads}", grads=grads, route="partials" if grads in ("g16", "none") else "atomic"))
    return cs


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def case_of(id):
    return CASES[CASE_IDS.index(id)]


def case_inputs(case, dtype):
    """-> the dict reference / emulate take; the e16 tensors are rounded here, once"""
    gen = torch.Generator().manual_seed(2000 + CASE_IDS.index(case["id"]))
    R, C, kind = case["R"], case["C"], case["kind"]

    def rn(*shape):
        return torch.randn(shape, generator=gen)

    x, y = rn(R, C), rn(R, C)
    if kind == "offset":
        x = x + 1000.0 * (1.0 + 0.2 * rn(R, 1))
    elif kind == "tiny":
        x, y = 1e-3 * x, 1e-3 * y
    elif kind == "constant":
        x, y = (3.0 * rn(R, 1)).expand(R, C).contiguous(), rn(R, 1).expand(R, C).contiguous()
    elif kind == "mixed":
        x[torch.arange(R), torch.randint(0, C, (R,), generator=gen)] = 300.0
    else:
        assert kind == "randn", kind
    gamma = 1.0 + 0.3 * rn(C)
    if case["gamma"] == "signed":
        gamma = rn(C)
        gamma[::3] = 0.0
    beta = 0.2 * rn(C)
    pe, g32, g16, gpe = rn(R, C).to(dtype), rn(R, C), rn(R, C).to(dtype), rn(R, C).to(dtype)
    grads = case["grads"]
    return dict(x=x, y=y.to(dtype) if case["y"] else None, gamma=gamma, beta=beta,
                pe=pe if case["outs"] == "pe" else None,
                g32=g32 if grads in ("g32", "all") else None, g16=g16 if grads in ("g16", "all") else None,
                gpe=gpe if grads in ("gpe", "all") else None,
                acc0=3.0 * rn(2 * C) if case["route"] == "atomic" else None)


def case_mask(case):
    return keep_mask(SEED, SALT, case["p"] if case["y"] else 0.0, case["R"], case["C"])


# ---- omnipq_layernorm_param_reduce ----------------------------------------------------------------------------------------

REDUCE_BLOCKS = (1, 2, 3, 4, 5, 12, 13, 16, 17, 512)


def reduce_inputs(blocks, C, seed):
    """synthetic partials with a wide dynamic range (ten decades), and the accumulator they are added to"""
    gen = torch.Generator().manual_seed(3000 + seed)
    part = torch.randn((blocks, 2 * C), generator=gen) * 10.0 ** (10.0 * torch.rand((blocks, 2 * C), generator=gen) - 5.0)
    return part, torch.randn(2 * C, generator=gen)


def reduce_items():
    """the mixed launch: 32 items, (blocks, C) of every kind side by side; the grid is sized by the widest"""
    Cs = (4, 1024, 8, 260, 288, 32, 516, 12)
    return [(REDUCE_BLOCKS[i % len(REDUCE_BLOCKS)] if i % 11 else 37, Cs[i % len(Cs)]) for i in range(32)]


def reduce_reference(part, out0):
    return out0.double() + part.double().sum(dim=0)


def reduce_bound(part, out0):
    blocks = part.shape[0]
    return MARGIN * (blocks // 16 + 8) * U32 * (part.double().abs().sum(dim=0) + out0.double().abs())


def reduce_emulate(part, out0, mutant=None):
    """a thread owns one column of one quarter of the blocks: four accumulators over an unrolled step of 16, a tail in steps
    of 4 into the first, the quarters folded pairwise, one atomic onto out"""
    blocks, c2 = part.shape
    red = []
    for q in range(4):
        acc = [torch.zeros(c2, dtype=F32) for _ in range(4)]
        b = q
        while b + 12 < blocks:
            for k in range(4):
                acc[k] = acc[k] + part[b + 4 * k]
            b += 16
        while b < blocks and mutant != "reduce_no_tail":
            acc[0] = acc[0] + part[b]
            b += 4
        red.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return out0 + ((red[0] + red[1]) + (red[2] + red[3]))


# ---- the flat kernels -----------------------------------------------------------------------------------------------------

FLAT_STRIDE = 4096 * 256 * 4           # elements one pass of the flat kernels' grid covers
ADDN_STRIDE = 2048 * 256 * 8           # ... of add_n's
FLAT_NS = (4, 4 * 37, FLAT_STRIDE + 4)
ADDN_NS = (8, 8 * 37, ADDN_STRIDE + 8)
ADDN_COUNTS = (1, 2, 5, 16)


def flat_inputs(n, dtype, seed):
    """e16 values with the edges in front: +-0, negative, the smallest subnormal and the largest, the smallest normal"""
    gen = torch.Generator().manual_seed(4000 + seed)
    h = torch.randn(n, generator=gen).to(dtype)
    tiny = torch.finfo(dtype).tiny
    sub = 2.0 ** -133 if dtype is torch.bfloat16 else 2.0 ** -24
    edge = torch.tensor([0.0, -0.0, sub, -sub, tiny - sub, tiny, -tiny, -1.5], dtype=torch.float64).to(dtype)
    k = min(n, edge.numel())
    h[n - k:] = edge[:k]                                    # at the END: the stride step's elements when n is one over
    if n >= 16:
        h[:8] = edge
    return h


def relu_dropout_reference(h, keep, p):
    hd = h.double()
    return torch.where(keep & (hd > 0), hd / (1.0 - as_f32(p)), torch.zeros_like(hd))


def relu_dropout_bwd_reference(h_out, d, p):
    return torch.where(h_out.double() > 0, d.double() / (1.0 - as_f32(p)), torch.zeros_like(d.double()))


def scaled_bound(ref, dtype):
    """one product with the f32 1 / (1 - p), one e16 store"""
    return MARGIN * ((3.0 * U32 + unit_roundoff(dtype)) * ref.abs() + abs_roundoff(dtype))


def sum_bound(terms, dtype):
    """f32 sum of the terms in turn, stored in dtype (None: left in f32)"""
    tot = sum(t.double() for t in terms)
    mag = sum(t.double().abs() for t in terms)
    b = (len(terms) - 1) * U32 * mag
    if dtype is not None:
        b = b + unit_roundoff(dtype) * tot.abs() + abs_roundoff(dtype)
    return tot, MARGIN * b


def relu_dropout_emulate(h, keep, p):
    v = h.to(F32)
    t = torch.where(v > 0, v, torch.zeros((), dtype=F32))
    if threshold(p):
        t = torch.where(keep, t * keep_inv_f32(p), torch.zeros((), dtype=F32))
    return t.to(h.dtype)


def relu_dropout_bwd_emulate(h_out, d, p, mutant=None):
    gate = (d.to(F32) > 0) if mutant == "relu_gate_from_grad" else (h_out.to(F32) > 0)
    return torch.where(gate, d.to(F32) * keep_inv_f32(p), torch.zeros((), dtype=F32)).to(d.dtype)


def add_n_emulate(srcs, out_dtype):
    acc = torch.zeros(srcs[0].shape, dtype=F32)
    for s in srcs:
        acc = acc + s.to(F32)
    return acc.to(out_dtype)


def addn_sources(count, n, dtype, seed):
    """count tensors of n elements from ONE draw: rolled and scaled by powers of two (exact in every type)"""
    gen = torch.Generator().manual_seed(5000 + seed)
    base = torch.randn(n, generator=gen)
    return [(base.roll(977 * i + 1) * 2.0 ** ((i % 5) - 2)).to(dtype) for i in range(count)]


# ---- pad / split / merge --------------------------------------------------------------------------------------------------

PAD_CASES = [dict(n=5, cin=0, k=8, ldx=4), dict(n=5, cin=3, k=32, ldx=4), dict(n=37, cin=3, k=32, ldx=7),
             dict(n=300, cin=32, k=32, ldx=40), dict(n=9, cin=5, k=9, ldx=6)]


def pad_reference(x_rows, cin, k, dtype):
    """x_rows (n, ldx) -> (n, k) in dtype: columns < cin converted (one rounding from f32), the others zero"""
    n = x_rows.shape[0]
    out = torch.zeros((n, k), dtype=dtype)
    out[:, :cin] = x_rows[:, :cin].to(dtype)
    return out


def split_cases():
    cs = []
    for c in (8, 288):
        for b, p in ((2, 7), (3, 1)):
            for p0 in sorted({0, 1, p - 1, p}):
                cs.append(dict(b=b, p=p, p0=p0, c=c))
    return cs


SPLIT_CASES = split_cases()


def split_reference(x, p0):
    """x (b, p, c) -> obj (b, p0, c), quad (b, p - p0, c)"""
    return x[:, :p0].contiguous(), x[:, p0:].contiguous()


def merge_terms(b, p, p0, c, g_obj, g_quad, g_joint, dtype):
    """-> the (b, p, c) terms merge_rows adds: [g_obj | g_quad] (zeros for a NULL one) and g_joint when given"""
    cat = torch.zeros((b, p, c), dtype=dtype)
    if g_obj is not None:
        cat[:, :p0] = g_obj
    if g_quad is not None:
        cat[:, p0:] = g_quad
    return [cat] if g_joint is None else [cat, g_joint]
