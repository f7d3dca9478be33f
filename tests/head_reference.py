"""Float64 reference of the prediction-head and vote decode kernels (csrc/head_ops.hip), the elementwise error bounds their
roundings allow, an independent restatement of the gradient descriptors, a CPU emulation of the kernels' f32 arithmetic, and
the case tables both suites walk.  Plain torch / numpy on the CPU.

The reference is evaluated in float64 from the tensors the kernels read: y / net rows in e16 (the library's 16-bit type);
base, means, seed_xyz, norm in f32; hr_scale as the f32 number the C ABI carries; every gradient in its own type through its
descriptor (`Grad`: storage, element strides sb / sk / s1 / s2 of the logical shape [B][K][n1][n2], n2), whose addressing
`grad_values` restates in numpy: element (b, k, j) lies at b sb + k sk + (j // n2) s1 + (j % n2) s2.

    object head   pick = FIRST index of the largest e16 size score (exact comparisons of stored values: bit-exact; -0 == +0)
                  center = y + base,  hr = hrn hr_scale,  sr = srn means,  pred = (sr + means)[pick]
                  obj, hs, hrn, ss, srn, sem: the bits of y
      backward    dy = [g_obj | g_center | g_hs | g_hrn + g_hr hr_scale | g_ss | g_srn + (g_sr + [cluster == pick] g_pred) means
                        | g_sem | 0 ...],  dbase = g_center (+ what the buffer held when accumulating)
    quad head     n = ||normals||_2 over the WHOLE tensor, normal = y / n, center = y + base; scores, size: the bits of y.
                  The reference keeps n unrounded; the kernel rounds it to e16 (torch.norm of a 16-bit tensor does).
      backward    with the norm the caller hands in (any f32): dnormal = g / n - y (sum g y) / n^3; the rest as above
    vote decode   vote_xyz = seed_xyz + offset,  v = seed + residual,  norm = ||v||_2 over channels,  out = v / norm
      backward    dv = (g - out <g, out>) / norm,  dnet = [g_xyz | dv | 0 ...],  dseed = dv
Non-finite size scores are out of scope: the kernel's `v > best` never picks a NaN, torch.argmax does.

Bounds.  u32 = 2^-24 per f32 operation, u = 2^-8 (bfloat16) or 2^-11 (half) per e16 store, eta = the absolute term of an
e16 store (decoder_reference.abs_roundoff).  |.| is elementwise.  To first order, every rounding on the longest path:

    center, vote_xyz   u32 |result|                                    one f32 addition of exact operands
    hr                 (u32 + u) |hr| + eta                            the product, the store
    sr                 u32 |sr|;   pred  u32 (|sr[pick]| + |pred|)     the product; the product and the sum
    dy, pass-through   0 from an e16 or absent gradient (conversions are exact), u |g| + eta from an f32 one
    dy, hrn columns    u32 (|g_hr hr_scale| + |g_hrn| + |g_hr hr_scale|) + u |dy| + eta
    dy, srn columns    t = g_sr + g_pred: u32 (|g_sr| + |g_pred|) |means| on the picked cluster, the product u32 |t means|,
                       the sum u32 (|g_srn| + |t means|); + u |dy| + eta
    dbase              0 (a copy);  accumulating: u32 (|before| + |g_center|)
    quad sum           a thread chains 12 fmas per trip of 1024 rows, a 6-step butterfly, 3 additions to fold the four
                       waves:  D = 12 ceil(R / 1024) + 9  roundings, each at most u32 times the sum of the |terms|
    n                  e_n = n (u32 (D / 2 + 1) + u) + eta             sum, sqrt, the e16 rounding
    normal             |normal| (e_n / n + u32 + u) + eta              the division, the store
    quad dnormal       S = sum g y:  e_S = D u32 sum |g y|;  s = S / n^3:  e_s = (e_S + 3 u32 |S|) / n^3
                       2 u32 (|g / n| + |y s|) + |y| e_s + u |dnormal| + eta   (from the terms, not from their difference)
    vote sums          channel-major: ceil(C / 8) fmas per thread + 8 partials;  rows: 8 fmas + the 6-step butterfly:  D
    vote norm          n u32 (D / 2 + 2):  v = seed + residual carries u32 |v| (one addition of exact operands), the sum of
                       squares (2 + D) u32, halved by the sqrt, the sqrt itself
    vote out           |out| u32 (D / 2 + 5): v, the norm, the reciprocal, the product;  e16 out / twin / rows: + u |out| + eta
    vote dv            d = <g, out>:  e_d = D u32 sum |g out|;
                       e_dv = (|out| e_d + u32 |out d| + 3 u32 (|g| + |out d|)) / norm: the product, the difference, the
                       reciprocal and the last product, from the magnitudes of g and out d;  e16: + u |dv| + eta
                       exactly 0 without a feature gradient;  dnet's xyz columns u |g_xyz| + eta, padding exact zeros

and all of it times MARGIN = 1.5 (decoder_reference.MARGIN, the constant of every reference module here) for what is not
modelled: second-order terms, fused multiply-adds that skip a rounding counted here, denormal results.
"""
import collections
import math

import numpy as np
import torch

from decoder_reference import MARGIN, U32, F32, abs_roundoff, as_f32, fmt, outside, ratios, unit_roundoff  # noqa: F401

F64 = torch.float64
_LANE = torch.arange(64)


def _z(*shape):
    return torch.zeros(shape, dtype=F64)


def _fma(a, b, c):
    """f32 fused multiply-add: the exact product of two f32 numbers fits a double, one more rounding to f32"""
    return (a.double() * b.double() + c.double()).float()


def _wave_sum(v):
    """(N, 64) -> (N,): the xor butterfly, every lane ends with the same bits"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, _LANE ^ o]
    return v[:, 0]


def norm_round_trips(norm32, dtype):
    """the quad head's stored norm is an e16 number: f32 -> e16 -> f32 gives back its bits"""
    return torch.equal(norm32.view(torch.int32), norm32.to(dtype).float().view(torch.int32))


# ---- gradient descriptors -------------------------------------------------------------------------------------------------

GRAD_KINDS = ("e16", "f32", "null", "scalar", "view")
Grad = collections.namedtuple("Grad", "storage sb sk s1 s2 n2 kind")


def make_grad(gen, B, K, n1, n2, kind, dtype, alt):
    """kind: e16 / f32 dense | null | scalar: one element, every stride 0 | view: the logical (B, K, n1, n2) seen through
    storage (B, n2, n1, K).  alt: scalar and view in e16 instead of f32"""
    if kind == "null":
        return Grad(None, 0, 0, 0, 0, n2, kind)
    dt = dtype if kind == "e16" or (kind in ("scalar", "view") and alt) else F32
    if kind == "scalar":
        return Grad(torch.randn(1, generator=gen).to(dt), 0, 0, 0, 0, n2, kind)
    vals = torch.randn(B * K * n1 * n2, generator=gen).to(dt)
    if kind == "view":
        return Grad(vals, n2 * n1 * K, 1, K, n1 * K, n2, kind)
    assert kind in ("e16", "f32"), kind
    return Grad(vals, K * n1 * n2, n1 * n2, n2, 1, n2, kind)


def grad_values(g, B, K, width):
    """-> float64 (B K, width): what the descriptor addresses, zeros for an absent gradient"""
    if g.storage is None:
        return _z(B * K, width)
    b = np.arange(B, dtype=np.int64)[:, None, None]
    k = np.arange(K, dtype=np.int64)[None, :, None]
    j = np.arange(width, dtype=np.int64)[None, None, :]
    off = b * g.sb + k * g.sk + (j // g.n2) * g.s1 + (j % g.n2) * g.s2
    flat = g.storage.double().numpy()
    assert off.min() >= 0 and off.max() < flat.size
    return torch.from_numpy(flat[off].reshape(B * K, width))


def grad_exact(g):
    """its conversion to e16 is exact: absent, or e16 itself"""
    return g.storage is None or g.storage.dtype is not F32


def rotated_kinds(rot, count):
    return [GRAD_KINDS[(rot + i) % 5] for i in range(count)]


def _store(mask, val, dtype):
    return mask * (unit_roundoff(dtype) * val.abs() + abs_roundoff(dtype))


# ---- object head ----------------------------------------------------------------------------------------------------------

HEAD_OUTPUTS = ("obj", "center", "hs", "hrn", "hr", "ss", "srn", "sr", "pred", "sem")       # HeadOut order
HEAD_BITS = ("obj", "hs", "hrn", "ss", "srn", "sem")                                        # pass-through: bit equality
HEAD_BOUNDED = ("center", "hr", "sr", "pred")
HEAD_F32 = ("center", "sr", "pred")
HEAD_N2 = (1, 1, 1, 1, 1, 1, 3, 3, 1, 1)
SCORE_KINDS = ("random", "tie", "equal", "last", "zeros")
DBASE_KINDS = ("null", "fresh", "acc")


def head_width(nh, ns, ncls):
    return 5 + 2 * nh + 4 * ns + ncls


def head_out_widths(nh, ns, ncls):
    return (2, 3, nh, nh, nh, ns, 3 * ns, 3 * ns, 3, ncls)


def head_cols(nh, ns, ncls):
    """{part of a row of y: (first column, columns)}"""
    return dict(obj=(0, 2), ctr=(2, 3), hs=(5, nh), hrn=(5 + nh, nh), ss=(5 + 2 * nh, ns), srn=(5 + 2 * nh + ns, 3 * ns),
                sem=(5 + 2 * nh + 4 * ns, ncls))


def head_inputs(dims, B, K, ldy, score, dtype, seed):
    """score: random | tie: the maximum at 0 and ns - 1 | equal | last: the maximum at ns - 1 | zeros: -0 at 0, +0 at ns - 1,
    the others negative.  The spare columns of the pitch are NaN: never read."""
    nh, ns, ncls = dims
    R, w = B * K, head_width(*dims)
    assert ldy >= w
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn((R, ldy), generator=gen).clamp(-3.0, 3.0)
    c = head_cols(*dims)["ss"][0]
    s = y[:, c:c + ns]
    if score == "tie":
        s[:, 0] = 3.5
        s[:, ns - 1] = 3.5
    elif score == "equal":
        s[:] = 0.75
    elif score == "last":
        s[:, ns - 1] = 3.5
    elif score == "zeros":
        s[:] = -(s.abs() + 0.125)
        s[:, 0] = -0.0
        s[:, ns - 1] = 0.0
    else:
        assert score == "random", score
    y = y.to(dtype)
    y[:, w:] = float("nan")
    return dict(dims=dims, B=B, K=K, ldy=ldy, y=y, base=torch.randn((R, 3), generator=gen),
                means=torch.rand((ns, 3), generator=gen) + 0.2, hr_scale=as_f32(math.pi / nh))


def head_grads(dims, B, K, rot, dtype, seed):
    """the ten output gradients, their kinds rotated by rot"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, (wd, n2, kind) in enumerate(zip(head_out_widths(*dims), HEAD_N2, rotated_kinds(rot, 10))):
        out.append(make_grad(gen, B, K, wd // n2, n2, kind, dtype, alt=bool((i + rot) % 2)))
    return out


def first_max(inp):
    """-> int64 (R,): the first index of the largest size score"""
    c, ns = head_cols(*inp["dims"])["ss"]
    s = inp["y"][:, c:c + ns].double().numpy()
    return torch.from_numpy(np.argmax(s == s.max(axis=1, keepdims=True), axis=1).astype(np.int64))


def _part(inp, name, t=None):
    c, n = head_cols(*inp["dims"])[name]
    return (inp["y"] if t is None else t)[:, c:c + n]


def head_reference(inp):
    """-> {output: float64, or the e16 bits for the pass-through outputs} + pick"""
    ns = inp["dims"][1]
    yd = inp["y"].double()
    pick = first_max(inp)
    means = inp["means"].double().reshape(1, 3 * ns)
    sr = _part(inp, "srn", yd) * means
    at = 3 * pick[:, None] + torch.arange(3)[None, :]
    ref = dict(pick=pick, center=_part(inp, "ctr", yd) + inp["base"].double(), hr=_part(inp, "hrn", yd) * inp["hr_scale"],
               sr=sr, pred=torch.gather(sr + means, 1, at), sr_pick=torch.gather(sr, 1, at))
    for name in HEAD_BITS:
        ref[name] = _part(inp, name).contiguous()
    return ref


def head_bounds(ref, dtype):
    b = dict(center=U32 * ref["center"].abs(), hr=U32 * ref["hr"].abs() + _store(1.0, ref["hr"], dtype),
             sr=U32 * ref["sr"].abs(), pred=U32 * (ref["sr_pick"].abs() + ref["pred"].abs()))
    return {k: MARGIN * v for k, v in b.items()}


def head_bwd_reference(inp, grads, lddy, dbase0=None):
    """grads: ten Grad in HeadOut order; dbase0: None, or the f32 (R, 3) the buffer holds when accumulating.
    -> dict(dy (R, lddy), dbase (R, 3), and what head_bwd_bounds needs)"""
    dims, B, K = inp["dims"], inp["B"], inp["K"]
    nh, ns, ncls = dims
    R, w = B * K, head_width(*dims)
    assert lddy >= w
    g = [grad_values(x, B, K, wd) for x, wd in zip(grads, head_out_widths(*dims))]
    ex = [0.0 if grad_exact(x) else 1.0 for x in grads]
    pick = first_max(inp)
    means = inp["means"].double().reshape(1, 3 * ns)
    on = (torch.arange(3 * ns)[None, :] // 3 == pick[:, None]).double()
    gp = g[8].repeat(1, ns) * on                                              # column 3 cluster + axis <- g_pred[axis]
    t = g[7] + gp
    tm, th = t * means, g[4] * inp["hr_scale"]
    dy = torch.cat([g[0], g[1], g[2], g[3] + th, g[5], g[6] + tm, g[9], _z(R, lddy - w)], dim=1)
    e32 = torch.cat([_z(R, 5 + nh), U32 * (2.0 * th.abs() + g[3].abs()), _z(R, ns),
                     U32 * ((g[7].abs() + gp.abs()) * on * means + 2.0 * tm.abs() + g[6].abs()), _z(R, ncls + lddy - w)], dim=1)
    one = torch.ones
    st = torch.cat([ex[0] * one(R, 2), ex[1] * one(R, 3), ex[2] * one(R, nh), one(R, nh), ex[5] * one(R, ns), one(R, 3 * ns),
                    ex[9] * one(R, ncls), _z(R, lddy - w)], dim=1).double()
    prior = _z(R, 3) if dbase0 is None else dbase0.double()
    return dict(dy=dy, e32=e32, st=st, dbase=prior + g[1], e_dbase=_z(R, 3) if dbase0 is None else U32 * (prior.abs() + g[1].abs()))


def head_bwd_bounds(ref, dtype):
    return dict(dy=MARGIN * (ref["e32"] + _store(ref["st"], ref["dy"], dtype)), dbase=MARGIN * ref["e_dbase"])


HEAD_MUTANTS = ("argmax_last", "hr_scale_on_hrn", "pred_no_means", "pred_pick_minus_1", "dy_pad_unwritten", "dbase_replace")
QUAD_MUTANTS = ("quad_drop_rows_ge_1024", "quad_count_clamped", "norm_not_rounded", "n2_for_n3", "dy_pad_unwritten",
                "dbase_replace")
VOTE_MUTANTS = ("vote_dot_wrong_point", "vote_no_projection", "rows_ignore_last_lane")
MUTANTS = tuple(dict.fromkeys(HEAD_MUTANTS + QUAD_MUTANTS + VOTE_MUTANTS))


def _pick_emulated(inp, mutant):
    s = _part(inp, "ss").float()
    best, bv = torch.zeros(s.shape[0], dtype=torch.int64), s[:, 0].clone()
    for c in range(1, s.shape[1]):
        better = (s[:, c] >= bv) if mutant == "argmax_last" else (s[:, c] > bv)
        best, bv = torch.where(better, torch.full_like(best, c), best), torch.where(better, s[:, c], bv)
    return best


def head_emulate(inp, dtype, mutant=None):
    """head_decode_body in f32"""
    assert mutant is None or mutant in MUTANTS
    ns = inp["dims"][1]
    pick = _pick_emulated(inp, mutant)
    means = inp["means"].reshape(1, 3 * ns)
    scale = torch.tensor(inp["hr_scale"], dtype=F32)
    sr = _part(inp, "srn").float() * means
    at = 3 * pick[:, None] + torch.arange(3)[None, :]
    got = dict(center=_part(inp, "ctr").float() + inp["base"], hr=(_part(inp, "hrn").float() * scale).to(dtype), sr=sr,
               pred=torch.gather(sr, 1, at) + torch.gather(means.expand_as(sr), 1, at))
    for name in HEAD_BITS:
        got[name] = _part(inp, name).contiguous()
    return got


def _dbase_emulated(g_center, dbase0, mutant):
    if dbase0 is None or mutant == "dbase_replace":
        return g_center.float()
    return dbase0 + g_center.float()


def _pad_emulated(R, n, mutant):
    return torch.full((R, n), float("nan") if mutant == "dy_pad_unwritten" else 0.0, dtype=F32)


def head_bwd_emulate(inp, grads, lddy, dbase0, dtype, mutant=None):
    """head_decode_bwd_body in f32 -> dict(dy e16 (R, lddy), dbase f32 (R, 3))"""
    assert mutant is None or mutant in MUTANTS
    dims, B, K = inp["dims"], inp["B"], inp["K"]
    nh, ns, ncls = dims
    R, w = B * K, head_width(*dims)
    g = [grad_values(x, B, K, wd).float() for x, wd in zip(grads, head_out_widths(*dims))]
    pick = _pick_emulated(inp, mutant)
    if mutant == "pred_pick_minus_1":
        pick = pick - 1
    means = inp["means"].reshape(1, 3 * ns)
    scale = torch.tensor(inp["hr_scale"], dtype=F32)
    on = torch.arange(3 * ns)[None, :] // 3 == pick[:, None]
    gp = torch.where(on, g[8].repeat(1, ns), torch.zeros((), dtype=F32))
    if mutant == "pred_no_means":
        srn = g[6] + g[7] * means + gp
    else:
        srn = g[6] + (g[7] + gp) * means
    hrn = (g[3] * scale + g[4]) if mutant == "hr_scale_on_hrn" else (g[3] + g[4] * scale)
    dy = torch.cat([g[0], g[1], g[2], hrn, g[5], srn, g[9], _pad_emulated(R, lddy - w, mutant)], dim=1).to(dtype)
    return dict(dy=dy, dbase=_dbase_emulated(g[1], dbase0, mutant))


def _head_cases():
    dims_all = ((1, 18, 18), (12, 10, 10), (1, 1, 1), (12, 18, 37))
    bks = ((1, 1), (1, 2), (3, 1), (2, 5), (3, 85))
    cs = []
    for d, dims in enumerate(dims_all):
        w = head_width(*dims)
        for i, (B, K) in enumerate(bks):
            score, rot = SCORE_KINDS[(i + 2 * d) % 5], (i + d) % 5
            cs.append(dict(id=f"head-w{w}-{B}x{K}-{score}-rot{rot}", dims=dims, B=B, K=K, score=score, rot=rot,
                           ldy=(w, (w + 7) // 8 * 8, (w + 7) // 8 * 8 + 8)[i % 3], lddy=(w, w + 3, w + 130)[(i + d) % 3],
                           dbase=DBASE_KINDS[(i + 2 * d) % 3], seed=100 + 5 * d + i))
    return cs


HEAD_CASES = _head_cases()


def dbase_prior(case, R):
    """None, or the f32 (R, 3) an accumulating call finds"""
    if case["dbase"] != "acc":
        return None
    return 3.0 * torch.randn((R, 3), generator=torch.Generator().manual_seed(case["seed"] + 50000))


def head_case_inputs(case, dtype):
    inp = head_inputs(case["dims"], case["B"], case["K"], case["ldy"], case["score"], dtype, case["seed"])
    return inp, head_grads(case["dims"], case["B"], case["K"], case["rot"], dtype, case["seed"] + 10000)


# ---- quad head ------------------------------------------------------------------------------------------------------------

QUAD_OUTPUTS = ("scores", "center", "normal", "size")
QUAD_WIDTHS = (2, 3, 3, 2)
QUAD_KINDS = ("randn", "dominated", "offset")
QUAD_RS = (1, 31, 32, 33, 255, 257, 1023, 1025, 1281, 2304)


def quad_depth(R):
    return 12 * ((R + 1023) // 1024) + 6 + 3


def quad_inputs(B, K, ldy, kind, dtype, seed):
    """kind: randn | dominated: rows 0, R // 2 and R - 1 are 2^11 times the others, the tensor's sum is theirs |
    offset: every component of the normals near 5"""
    R = B * K
    assert ldy >= 10
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn((R, ldy), generator=gen)
    if kind == "dominated":
        scale = torch.full((R, 1), 2.0 ** -6)
        scale[[0, R // 2, R - 1]] = 32.0
        y[:, 5:8] *= scale
    elif kind == "offset":
        y[:, 5:8] = 5.0 + 2.0 ** -6 * y[:, 5:8]
    else:
        assert kind == "randn", kind
    y = y.to(dtype)
    y[:, 10:] = float("nan")
    return dict(B=B, K=K, ldy=ldy, y=y, base=torch.randn((R, 3), generator=gen))


def quad_grads(B, K, rot, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return [make_grad(gen, B, K, wd, 1, kind, dtype, alt=bool((i + rot) % 2))
            for i, (wd, kind) in enumerate(zip(QUAD_WIDTHS, rotated_kinds(rot, 4)))]


def quad_reference(inp):
    yd = inp["y"].double()
    nrm = yd[:, 5:8].pow(2).sum().sqrt().reshape(1)
    return dict(norm=nrm, center=yd[:, 2:5] + inp["base"].double(), normal=yd[:, 5:8] / nrm,
                scores=inp["y"][:, 0:2].contiguous(), size=inp["y"][:, 8:10].contiguous())


def quad_bounds(ref, dtype):
    R = ref["center"].shape[0]
    n, u, eta = ref["norm"], unit_roundoff(dtype), abs_roundoff(dtype)
    e_n = n * (U32 * (quad_depth(R) / 2.0 + 1.0) + u) + eta
    b = dict(norm=e_n, center=U32 * ref["center"].abs(), normal=ref["normal"].abs() * (e_n / n + U32 + u) + eta)
    return {k: MARGIN * v for k, v in b.items()}


def quad_bwd_reference(inp, grads, lddy, norm_in, dbase0=None):
    """norm_in: the f32 number the call is handed (a Python float)"""
    B, K = inp["B"], inp["K"]
    R = B * K
    assert lddy >= 10
    g = [grad_values(x, B, K, wd) for x, wd in zip(grads, QUAD_WIDTHS)]
    ex = [0.0 if grad_exact(x) else 1.0 for x in grads]
    y = inp["y"].double()[:, 5:8]
    n = as_f32(norm_in)
    S, absS = (g[2] * y).sum(), (g[2] * y).abs().sum()
    s = S / n ** 3
    dn = g[2] / n - y * s
    e_s = (quad_depth(R) * U32 * absS + 3.0 * U32 * S.abs()) / n ** 3
    e32 = torch.cat([_z(R, 5), 2.0 * U32 * ((g[2] / n).abs() + (y * s).abs()) + y.abs() * e_s, _z(R, lddy - 8)], dim=1)
    one = torch.ones
    st = torch.cat([ex[0] * one(R, 2), ex[1] * one(R, 3), one(R, 3), ex[3] * one(R, 2), _z(R, lddy - 10)], dim=1).double()
    prior = _z(R, 3) if dbase0 is None else dbase0.double()
    return dict(dy=torch.cat([g[0], g[1], dn, g[3], _z(R, lddy - 10)], dim=1), e32=e32, st=st, dbase=prior + g[1],
                e_dbase=_z(R, 3) if dbase0 is None else U32 * (prior.abs() + g[1].abs()))


quad_bwd_bounds = head_bwd_bounds


def _quad_sum(a, b, mutant):
    """sum a b over (R, 3) the way a workgroup of 256 threads forms it: thread t chains the rows t + 256 u + 1024 trip"""
    R = a.shape[0]
    t = torch.arange(256)
    acc = torch.zeros(256, dtype=F32)
    for trip in range((R + 1023) // 1024):
        if trip and mutant == "quad_drop_rows_ge_1024":
            break
        r0 = t + 1024 * trip
        for u in range(4):
            r = r0 + 256 * u
            live = (r0 < R) if mutant == "quad_count_clamped" else (r < R)
            rc = torch.where(r < R, r, r0).clamp(max=R - 1)
            for c in range(3):
                av = torch.where(live, a[rc, c], torch.zeros((), dtype=F32))
                acc = _fma(av, b[rc, c], acc)
    red = _wave_sum(acc.reshape(4, 64))
    return (red[0] + red[1]) + (red[2] + red[3])


def quad_emulate(inp, dtype, mutant=None):
    assert mutant is None or mutant in MUTANTS
    v = inp["y"][:, 5:8].float()
    nrm = torch.sqrt(_quad_sum(v, v, mutant))
    if mutant != "norm_not_rounded":
        nrm = nrm.to(dtype).float()
    return dict(norm=nrm.reshape(1), center=inp["y"][:, 2:5].float() + inp["base"], normal=(v / nrm).to(dtype),
                scores=inp["y"][:, 0:2].contiguous(), size=inp["y"][:, 8:10].contiguous())


def quad_bwd_emulate(inp, grads, lddy, norm_in, dbase0, dtype, mutant=None):
    assert mutant is None or mutant in MUTANTS
    B, K = inp["B"], inp["K"]
    R = B * K
    g = [grad_values(x, B, K, wd).float() for x, wd in zip(grads, QUAD_WIDTHS)]
    y = inp["y"][:, 5:8].float()
    nrm = torch.tensor(norm_in, dtype=F32)
    s = _quad_sum(g[2], y, mutant) / ((nrm * nrm) if mutant == "n2_for_n3" else (nrm * nrm * nrm))
    dy = torch.cat([g[0], g[1], g[2] / nrm - y * s, g[3], _pad_emulated(R, lddy - 10, mutant)], dim=1).to(dtype)
    return dict(dy=dy, dbase=_dbase_emulated(g[1], dbase0, mutant))


def _quad_cases():
    cs = []
    for ri, R in enumerate(QUAD_RS):
        for ki, kind in enumerate(QUAD_KINDS):
            n = 3 * ri + ki
            B, K = (3, 427) if R == 1281 else ((1, R) if (ri + ki) % 2 == 0 else (R, 1))
            cs.append(dict(id=f"quad-R{R}-{kind}", R=R, B=B, K=K, kind=kind, ldy=(10, 32)[(n + ri) % 2],
                           lddy=(10, 16, 35)[(ri + ki) % 3], rot=n % 5, dbase=DBASE_KINDS[(ri + 2 * ki) % 3],
                           norm="own" if n % 2 == 0 else "any", seed=200 + n))
    return cs


QUAD_CASES = _quad_cases()


def quad_case_inputs(case, dtype):
    inp = quad_inputs(case["B"], case["K"], case["ldy"], case["kind"], dtype, case["seed"])
    return inp, quad_grads(case["B"], case["K"], case["rot"], dtype, case["seed"] + 10000)


def quad_case_norm(case, inp, dtype):
    """the f32 norm the backward call is handed: the e16-rounded norm of the tensor ("own"), or just some f32 near it"""
    n = float(quad_reference(inp)["norm"])
    return float(torch.tensor(n).to(dtype).float()) if case["norm"] == "own" else as_f32(1.37 * n)


# ---- pair and group -------------------------------------------------------------------------------------------------------
# (B, Kh, Kq): (Rh, Rq) = (3, 33): an odd half-block, a partly filled quad block; (170, 1281): the quad sum's second trip
PAIR_CASES = (dict(id="pair-3-33", B=3, Kh=1, Kq=11, dims=(1, 18, 18), score="tie", rot=1, seed=301),
              dict(id="pair-170-1281", B=1, Kh=170, Kq=1281, dims=(12, 18, 37), score="random", rot=3, seed=302))
GROUP_CASE = dict(id="group-5", n=5, B=3, Kh=5, Kq=11, dims=(1, 18, 18), seed=310)       # five stages: two launches


def sink_reference(centre_grads, prior):
    """centre_grads: float64 (R, 3) per stage; prior: f32 (R, 3) or None -> (sum, bound): one f32 addition per term"""
    terms = ([] if prior is None else [prior.double()]) + list(centre_grads)
    tot, mag = sum(terms), sum(t.abs() for t in terms)
    return tot, MARGIN * (len(terms) - 1) * U32 * mag


# ---- vote decode ----------------------------------------------------------------------------------------------------------

VOTE_LAYOUTS = ("cm-f32", "cm-e16", "pm-f32", "pm-e16")     # seed features (b, c, k): channel-major or position-major storage
VOTE_NULLS = ("none", "g_xyz", "g_feat", "dseed")
VOTE_BKS = ((1, 1), (2, 31), (1, 32), (3, 33), (2, 77))
VOTE_CS = (1, 8, 67, 288, 320)
ROWS_NS = (1, 3, 4, 5, 131)
ROWS_CS = (8, 288, 320)


def vote_depth(C, rows):
    return 8 + 6 if rows else (C + 7) // 8 + 8


def vote_ld(C, by8):
    """the smallest pitch that is / is not a multiple of 8"""
    if by8:
        return (C + 3 + 7) // 8 * 8
    return C + 4 if (C + 4) % 8 else C + 5


def vote_inputs(N, C, ld, feat_dtype, dtype, seed):
    """point-major: net e16 (N, ld) = [offset 3 | residual C | NaN ...], seed_xyz f32 (N, 3), seed features (N, C)"""
    assert ld >= C + 3
    gen = torch.Generator().manual_seed(seed)
    net = torch.randn((N, ld), generator=gen).to(dtype)
    net[:, C + 3:] = float("nan")
    return dict(net=net, seed_xyz=torch.randn((N, 3), generator=gen), seed=torch.randn((N, C), generator=gen).to(feat_dtype))


def vote_reference(inp):
    C = inp["seed"].shape[1]
    nd = inp["net"].double()
    v = inp["seed"].double() + nd[:, 3:3 + C]
    norm = v.pow(2).sum(dim=1).sqrt()
    return dict(vote_xyz=inp["seed_xyz"].double() + nd[:, :3], norm=norm, out=v / norm[:, None])


def vote_bounds(ref, dtype, depth, out_e16):
    out = ref["out"]
    e = U32 * (depth / 2.0 + 5.0) * out.abs()
    b = dict(vote_xyz=U32 * ref["vote_xyz"].abs(), norm=U32 * (depth / 2.0 + 2.0) * ref["norm"],
             out=e + _store(1.0 if out_e16 else 0.0, out, dtype), twin=e + _store(1.0, out, dtype))
    return {k: MARGIN * v for k, v in b.items()}


def vote_bwd_inputs(inp, feat_dtype, ldd, null, seed):
    """the backward's operands from the forward's reference: out in the features' type, norm in f32; null: which optional
    pointer is NULL"""
    N, C = inp["seed"].shape
    assert ldd >= C + 3
    gen = torch.Generator().manual_seed(seed)
    ref = vote_reference(inp)
    g_xyz, g = torch.randn((N, 3), generator=gen), torch.randn((N, C), generator=gen).to(feat_dtype)
    return dict(out=ref["out"].to(feat_dtype), norm=ref["norm"].float(), g_xyz=None if null == "g_xyz" else g_xyz,
                g=None if null == "g_feat" else g, ldd=ldd, dseed=null != "dseed")


def vote_bwd_reference(bi):
    o, norm = bi["out"].double(), bi["norm"].double()[:, None]
    N, C = o.shape
    g = _z(N, C) if bi["g"] is None else bi["g"].double()
    gx = _z(N, 3) if bi["g_xyz"] is None else bi["g_xyz"].double()
    dot = (g * o).sum(dim=1, keepdim=True)
    dv = (g - o * dot) / norm
    return dict(dv=dv, gx=gx, dnet=torch.cat([gx, dv, _z(N, bi["ldd"] - 3 - C)], dim=1), o=o, g=g, dot=dot, norm=norm,
                absdot=(g * o).abs().sum(dim=1, keepdim=True), has_g=bi["g"] is not None, has_gx=bi["g_xyz"] is not None)


def vote_bwd_bounds(ref, dtype, depth, seed_e16):
    o, g, dv = ref["o"].abs(), ref["g"].abs(), ref["dv"]
    od = o * ref["dot"].abs()
    e = (o * depth * U32 * ref["absdot"] + U32 * od + 3.0 * U32 * (g + od)) / ref["norm"]
    has_g, has_gx = float(ref["has_g"]), float(ref["has_gx"])
    pad = ref["dnet"].shape[1] - 3 - dv.shape[1]
    b = dict(dseed=e + _store(has_g if seed_e16 else 0.0, dv, dtype),
             dnet=torch.cat([_store(has_gx, ref["gx"], dtype), e + _store(has_g, dv, dtype), _z(dv.shape[0], pad)], dim=1))
    return {k: MARGIN * v for k, v in b.items()}


def _vote_sum(a, b, rows, mutant):
    """sum_c a b per point, (N, C) -> (N,): channel-major kernels: thread cg of 8 chains the channels cg + 8 u, the 8 partials
    are added in turn; rows kernels: lane l chains the channels 8 l .. 8 l + 7, then the butterfly"""
    N, C = a.shape
    if rows:
        lanes = C // 8 - (1 if mutant == "rows_ignore_last_lane" else 0)
        A, Bm = a.reshape(N, C // 8, 8), b.reshape(N, C // 8, 8)
        acc = torch.zeros((N, 64), dtype=F32)
        for e in range(8):
            acc[:, :lanes] = _fma(A[:, :lanes, e], Bm[:, :lanes, e], acc[:, :lanes])
        return _wave_sum(acc)
    steps = (C + 7) // 8
    pad = torch.zeros((N, 8 * steps - C), dtype=F32)
    A, Bm = torch.cat([a, pad], dim=1).reshape(N, steps, 8), torch.cat([b, pad], dim=1).reshape(N, steps, 8)
    part = torch.zeros((N, 8), dtype=F32)
    for s in range(steps):
        part = _fma(A[:, s], Bm[:, s], part)
    tot = torch.zeros(N, dtype=F32)
    for cg in range(8):
        tot = tot + part[:, cg]
    return tot


def vote_emulate(inp, dtype, rows, out_e16, mutant=None):
    assert mutant is None or mutant in MUTANTS
    C = inp["seed"].shape[1]
    x = inp["net"].float()
    t = inp["seed"].float() + x[:, 3:3 + C]
    n = torch.sqrt(_vote_sum(t, t, rows, mutant))
    o = t * (1.0 / n)[:, None]
    return dict(vote_xyz=inp["seed_xyz"] + x[:, :3], norm=n, out=o.to(dtype) if out_e16 else o, twin=o.to(dtype))


def vote_bwd_emulate(bi, dtype, rows, seed_e16, mutant=None):
    assert mutant is None or mutant in MUTANTS
    o = bi["out"].float()
    N, C = o.shape
    g = torch.zeros((N, C), dtype=F32) if bi["g"] is None else bi["g"].float()
    gx = torch.zeros((N, 3), dtype=F32) if bi["g_xyz"] is None else bi["g_xyz"]
    dot = _vote_sum(g, o, rows, mutant)
    if mutant == "vote_dot_wrong_point":
        dot = dot.roll(-1)
    rn = (1.0 / bi["norm"])[:, None]
    t = g * rn if mutant == "vote_no_projection" else (g - o * dot[:, None]) * rn
    return dict(dnet=torch.cat([gx, t, torch.zeros((N, bi["ldd"] - 3 - C), dtype=F32)], dim=1).to(dtype),
                dseed=t.to(dtype) if seed_e16 else t)


def _vote_cases():
    cs = []
    for bi, (B, K) in enumerate(VOTE_BKS):
        for ci, C in enumerate(VOTE_CS):
            n = 5 * bi + ci
            cs.append(dict(id=f"vote-{B}x{K}-C{C}", B=B, K=K, C=C, ld=vote_ld(C, (bi + ci) % 2 == 0),
                           ldd=vote_ld(C, (bi + ci) % 2 == 1), layout=VOTE_LAYOUTS[(n + bi) % 4], null=VOTE_NULLS[(bi + 2 * ci) % 4],
                           seed=400 + n))
    return cs


def _rows_cases():
    cs = []
    for ri, N in enumerate(ROWS_NS):
        for ci, C in enumerate(ROWS_CS):
            n = 3 * ri + ci
            cs.append(dict(id=f"rows-{N}-C{C}", N=N, C=C, ldn=C + (8, 16)[(ri + ci) % 2], ldd=C + (16, 8)[ri % 2],
                           null=VOTE_NULLS[n % 4], seed=500 + n))
    return cs


VOTE_CASES = _vote_cases()
ROWS_CASES = _rows_cases()
ALL_CASES = HEAD_CASES + QUAD_CASES + VOTE_CASES + ROWS_CASES


def case_of(id):
    return next(c for c in ALL_CASES if c["id"] == id)


def vote_case_inputs(case, dtype):
    """-> forward and backward operands (point-major), the features' type"""
    ft = dtype if case["layout"].endswith("e16") else F32
    inp = vote_inputs(case["B"] * case["K"], case["C"], case["ld"], ft, dtype, case["seed"])
    return inp, vote_bwd_inputs(inp, ft, case["ldd"], case["null"], case["seed"] + 10000), ft


def rows_case_inputs(case, dtype):
    inp = vote_inputs(case["N"], case["C"], case["ldn"], dtype, dtype, case["seed"])
    return inp, vote_bwd_inputs(inp, dtype, case["ldd"], case["null"], case["seed"] + 10000)


def to_channel_major(x, B, K):
    """point-major (B K, C) -> (B, C, K) contiguous"""
    return x.reshape(B, K, -1).permute(0, 2, 1).contiguous()


def to_point_major(x):
    """(B, C, K) -> (B K, C)"""
    B, C, K = x.shape
    return x.permute(0, 2, 1).reshape(B * K, C).contiguous()
