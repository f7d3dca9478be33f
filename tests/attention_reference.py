"""Float64 reference of the attention kernels (csrc/attention.hip), the elementwise error bounds their roundings allow,
a CPU emulation of the kernels' arithmetic, and the case table both suites walk.  Plain torch on the CPU.

Everything here is HEAD-MAJOR: q, dO (B, L, D); k, v (B, S, D); B = batch * heads; keep mask (B, L, S) of 0 / 1 or None.
The reference is evaluated in float64 from the e16-ROUNDED inputs (the tensors the kernels read), with

    c = D^-0.5, s = c q k^T, P = softmax(s), M = mask / (1 - p) (ones without dropout), Pd = P * M
    O = Pd v,  lse2 = log2 sum_k 2^(s log2 e)
    dV = Pd^T dO,  dP = (dO v^T) * M,  delta = rowsum(P * dP),  dS = P * (dP - delta),  dQ = c dS k,  dK = c dS^T q

Bounds (`bounds`).  u = unit roundoff of the element type (2^-8 bfloat16, 2^-11 half); eta = an absolute term per rounding
(0 for bfloat16, whose subnormals sit at 1e-38; half's subnormal spacing 2^-24).  The kernels round (attention.hip,
`Numerics`): P to e16 before the second contraction, O on store, dS to e16 before its contractions, every gradient on store,
and they compute delta from the STORED (rounded) O.  To first order:

    O   u (Pd |v|) + u |O|                         every rounded P moves O by at most u P M |v|; then the store
    dV  u (Pd^T |dO|) + u |dV|
    dS  E = u (|dS| + P * rowsum_d(|dO| |O|))      the rounding of dS; delta from an O that is off by u |O| per channel
    dQ  c (E |k|) + u |dQ|
    dK  c (E^T |q|) + u |dK|
    half only: + eta per kept rounded P: the forward rounds the UN-normalised p <= 1, so eta (keep |v|) / l with the row's
    denominator l = sum_k 2^(s2 - max s2) -- an upper bound, a wave's running maximum is never above the row's; the dK/dV
    kernel rounds the normalised P: eta (keep^T |dO|); + eta per rounded dS: c eta sum|k| resp. c eta sum|q|; + eta per
    stored element.

and all of it times MARGIN = 1.5 for what is not modelled: f32 accumulation (at most terms * 2^-24 of the same absolute
sums), the hardware exp2, second-order terms.

    lse2   |got - ref| <= 1e-5 max(1, log2 e c max_k sum_d |q_d k_d|)
    delta  against sum_d dO O over the stored O: <= 2^-20 sum_d |dO O|
"""
import math

import torch

LOG2E = 1.4426950408889634
MARGIN = 1.5
OUTPUTS = ("O", "lse2", "delta", "dQ", "dK", "dV")


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def abs_roundoff(dtype):
    return {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24}[dtype]


def reference(q, k, v, do, mask=None, p=0.0):
    """float64 evaluation from e16 (or any) tensors; -> dict of float64 tensors, the intermediates included"""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    D = q.shape[-1]
    c = D ** -0.5
    s = c * q @ k.transpose(1, 2)
    smax = s.max(dim=2, keepdim=True).values
    e = torch.exp(s - smax)
    l = e.sum(dim=2, keepdim=True)                      # the row's denominator relative to its maximum: >= 1
    P = e / l
    keep = torch.ones_like(P) if mask is None else mask.double()
    M = keep / (1.0 - p)
    Pd = P * M
    O = Pd @ v
    lse2 = ((smax + torch.log(l)) * LOG2E).squeeze(2)
    dV = Pd.transpose(1, 2) @ do
    dP = (do @ v.transpose(1, 2)) * M
    delta = (P * dP).sum(dim=2, keepdim=True)
    dS = P * (dP - delta)
    dQ = c * dS @ k
    dK = c * dS.transpose(1, 2) @ q
    return dict(O=O, lse2=lse2, dV=dV, dQ=dQ, dK=dK, delta=delta.squeeze(2), P=P, Pd=Pd, dS=dS, keep=keep, l=l, c=c,
                q=q, k=k, v=v, do=do)


def bounds(ref, dtype, o_stored=None):
    """-> {output: float64 bound per element}.  o_stored: the O the backward read (its delta is bounded against that
    tensor); None = the reference's own O."""
    u, eta = unit_roundoff(dtype), abs_roundoff(dtype)
    q, k, v, do, c = ref["q"], ref["k"], ref["v"], ref["do"], ref["c"]
    P, Pd, dS, keep = ref["P"], ref["Pd"], ref["dS"], ref["keep"]
    kT = keep.transpose(1, 2)
    O = ref["O"]
    b = {}
    b["O"] = u * (Pd @ v.abs()) + u * O.abs() + eta * ((keep / ref["l"]) @ v.abs()) + eta
    b["dV"] = u * (Pd.transpose(1, 2) @ do.abs()) + u * ref["dV"].abs() + eta * (kT @ do.abs()) + eta
    E = u * (dS.abs() + P * (do.abs() * O.abs()).sum(dim=2, keepdim=True))
    b["dQ"] = c * (E @ k.abs()) + u * ref["dQ"].abs() + c * eta * k.abs().sum(dim=1, keepdim=True) + eta
    b["dK"] = c * (E.transpose(1, 2) @ q.abs()) + u * ref["dK"].abs() + c * eta * q.abs().sum(dim=1, keepdim=True) + eta
    for name in ("O", "dV", "dQ", "dK"):
        b[name] = MARGIN * b[name]
    qk = (q.abs().unsqueeze(2) * k.abs().unsqueeze(1)).sum(dim=3).max(dim=2).values          # max_k sum_d |q_d k_d|
    b["lse2"] = 1e-5 * torch.clamp(LOG2E * c * qk, min=1.0)
    osd = O if o_stored is None else o_stored.double()
    b["delta"] = 2.0 ** -20 * (do * osd).abs().sum(dim=2)
    return b


def delta_of(do, o_stored):
    return (do.double() * o_stored.double()).sum(dim=2)


def ratios(got, ref, bnd, o_stored=None):
    """got: {output: tensor}.  -> {output: (largest error / bound, number of elements outside)}; an element that is not
    finite, or off where the bound is zero, counts as outside with ratio inf."""
    out = {}
    for name, g in got.items():
        want = delta_of(ref["do"], o_stored) if name == "delta" and o_stored is not None else ref[name]
        err = (g.double() - want).abs()
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


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def make_inputs(L, S, N, H, D, kind="randn", seed=0, dtype=torch.bfloat16, do_scale=1.0):
    """-> q, dO (B, L, D), k, v (B, S, D) in `dtype` (the rounding to e16 happens here, once).  kind:
    randn   q, k = 1.5 randn: logits within a few units
    big     q, k = 6 randn: logits of +-100 and more, the maximum moves around
    inc     key norms increasing along S: every key block raises every query's maximum
    dec     the same keys in reverse: no block after a wave's first raises it
    last    one dominant key, at index S - 1
    equal   all keys of a (batch, head) equal: uniform softmax, lse2 = s log2 e + log2 S
    neg80   (batch, head) 0 has all scores near -80, the others as randn"""
    gen = torch.Generator().manual_seed(1000 + seed)
    B = N * H

    def rn(*shape):
        return torch.randn(shape, generator=gen)

    amp = 6.0 if kind == "big" else 1.5
    q, k, v, do = amp * rn(B, L, D), amp * rn(B, S, D), rn(B, S, D), rn(B, L, D) * do_scale
    if kind in ("inc", "dec", "last", "neg80"):
        w = torch.ones(D) / math.sqrt(D)                                # unit direction: q.k = (q.w)(k.w) + noise
        bq = (0.75 + 0.5 * torch.rand((B, L, 1), generator=gen)) * math.sqrt(D)         # c * (q.w) in [0.75, 1.25]
        if kind in ("inc", "dec"):
            a = torch.linspace(0.0, 40.0, S).reshape(1, S, 1)           # logits rise by ~40 over the S keys
            if kind == "dec":
                a = a.flip(1)
            q, k = bq * w + 0.3 * rn(B, L, D), a * w + 0.05 * rn(B, S, D)  # key to key: +0.3 +- 0.07
        elif kind == "last":
            q = bq * w + 0.3 * rn(B, L, D)
            k = 0.5 * rn(B, S, D)
            k[:, S - 1] = 30.0 * w + 0.3 * rn(B, D)
        else:
            q[0], k[0] = (bq * w + 0.05 * rn(B, L, D))[0], (-80.0 * w + 0.05 * rn(B, S, D))[0]
    elif kind == "equal":
        k = k[:, :1].expand(B, S, D).clone()
    else:
        assert kind in ("randn", "big"), kind
    return tuple(t.to(dtype) for t in (q, k, v, do))


def bernoulli_mask(B, L, S, p, seed):
    """a keep mask for the CPU checks (on the GPU the mask is the one the kernels drew)"""
    gen = torch.Generator().manual_seed(77 + seed)
    return (torch.rand((B, L, S), generator=gen) >= p).to(torch.uint8)


# ---- the kernels' arithmetic on the CPU -----------------------------------------------------------------------------------

MUTANTS = ("drop_last_key", "ln_lse", "delta_no_mask", "bwd_other_mask", "dk_no_scale", "half_swap", "no_rescale")


def _swap_halves(x):
    """keys 4h..4h+3 of each 8 exchanged between the two lane halves (last axis, a multiple of 8 long)"""
    shp = x.shape
    return x.reshape(*shp[:-1], shp[-1] // 8, 2, 4).flip(-2).reshape(shp)


def emulate(q, k, v, do, mask=None, p=0.0, mutant=None, mask_bwd=None):
    """f32 arithmetic with the kernels' roundings and the forward's block structure: four waves take the key blocks of 32
    in turn, each with a running maximum (online softmax), P is rounded to e16 per block, the waves are merged, O is
    rounded on store; backward: delta from the stored O, P = 2^(s2 - lse2), dS and P rounded to e16, gradients rounded
    on store.  mutant: one of MUTANTS, the defect the bounds must catch.  -> {output: tensor}"""
    assert mutant is None or mutant in MUTANTS
    dt = q.dtype
    B, L, D = q.shape
    S = k.shape[1]
    f32 = torch.float32

    def rnd(x):
        return x.to(dt).to(f32)

    qf, kf, vf, dof = (t.to(f32) for t in (q, k, v, do))
    c = torch.tensor(1.0 / math.sqrt(D), dtype=f32)
    sl2 = c * torch.tensor(LOG2E, dtype=f32)
    keep_inv = torch.tensor(1.0, dtype=f32) / (torch.tensor(1.0, dtype=f32) - torch.tensor(p, dtype=f32))
    keep = torch.ones((B, L, S), dtype=f32) if mask is None else mask.to(f32)
    keep_b = keep if mask_bwd is None else mask_bwd.to(f32)
    if mutant == "bwd_other_mask":
        assert mask_bwd is not None
    Spad = (S + 31) // 32 * 32

    def pad(x, axis):                                   # zero rows up to a whole block, as the buffer loads return
        shp = list(x.shape)
        shp[axis] = Spad - S
        return torch.cat([x, torch.zeros(shp, dtype=x.dtype)], dim=axis)

    kp, vp, keepp = pad(kf, 1), pad(vf, 1), pad(keep, 2)
    s_valid = S - 1 if mutant == "drop_last_key" and S % 32 else S
    ms, ls, accs = [], [], []
    for wave in range(4):
        m = torch.full((B, L), -1e30, dtype=f32)
        lsum = torch.zeros((B, L), dtype=f32)
        acc = torch.zeros((B, L, D), dtype=f32)
        for k0 in range(wave * 32, Spad, 128):
            st = qf @ kp[:, k0:k0 + 32].transpose(1, 2)
            ok = (torch.arange(k0, k0 + 32) < s_valid).reshape(1, 1, 32)
            s2 = torch.where(ok, st * sl2, torch.tensor(-1e30, dtype=f32))
            m_new = torch.maximum(m, s2.max(dim=2).values)
            alpha = torch.exp2(m - m_new)
            pe = torch.where(ok, torch.exp2(s2 - m_new.unsqueeze(2)), torch.tensor(0.0, dtype=f32))
            lsum = lsum * alpha + pe.sum(dim=2)
            if mutant != "no_rescale":
                acc = acc * alpha.unsqueeze(2)
            m = m_new
            p16 = rnd(pe * keepp[:, :, k0:k0 + 32] * keep_inv)
            if mutant == "half_swap":
                p16 = _swap_halves(p16)
            acc = acc + p16 @ vp[:, k0:k0 + 32]
        ms.append(m), ls.append(lsum), accs.append(acc)
    mstar = torch.stack(ms).max(dim=0).values
    fs = [torch.exp2(m - mstar) for m in ms]
    l = sum(lw * f for lw, f in zip(ls, fs))
    o = sum(a * f.unsqueeze(2) for a, f in zip(accs, fs))
    O = rnd(o / l.unsqueeze(2))
    lse2 = mstar + torch.log2(l)
    if mutant == "ln_lse":
        lse2 = lse2 * math.log(2.0)
    # backward
    st = qf @ kf.transpose(1, 2)
    P = torch.exp2(st * sl2 - (mstar + torch.log2(l)).unsqueeze(2))
    dpu = dof @ vf.transpose(1, 2)
    delta = (dof * O).sum(dim=2)
    dl = (P * dpu).sum(dim=2) if mutant == "delta_no_mask" else delta
    dp = dpu * keep_b * keep_inv
    ds16 = rnd(P * (dp - dl.unsqueeze(2)))
    pt16 = rnd(P * keep_b * keep_inv)
    dQ = rnd((ds16 @ kf) * c)
    dK = rnd((ds16.transpose(1, 2) @ qf) * (1.0 if mutant == "dk_no_scale" else c))
    dV = rnd(pt16.transpose(1, 2) @ dof)
    return dict(O=O.to(dt), lse2=lse2, delta=delta, dQ=dQ.to(dt), dK=dK.to(dt), dV=dV.to(dt))


# ---- the cases ------------------------------------------------------------------------------------------------------------
# dict(id, L, S, N, H, D, p, kind, layout, dtype, do_scale).  Layouts (GPU suite; the arithmetic does not depend on them):
#   contig      (tokens, batch, embed)
#   pitch4      rows of E + 4 elements: 8-byte but not 16-byte aligned
#   self        packed self attention: q|k|v side by side, token stride 3E, batch stride L 3E; gradients likewise
#   cross       packed cross attention: q E / L E, k|v 2E / S 2E; gradients likewise
#   own         o, dq, dk and dv each with a pitch and a batch order of its own

def _case(id, L, S, N=1, H=2, D=36, p=0.0, kind="randn", layout="contig", dtype=torch.bfloat16, do_scale=1.0):
    return dict(id=id, L=L, S=S, N=N, H=H, D=D, p=p, kind=kind, layout=layout, dtype=dtype, do_scale=do_scale)


def _cases():
    cs = []
    for L in (1, 31, 32, 33, 65):                       # S: one key; waves without keys; one full iteration; a second
        for S in (1, 31, 33, 45, 128, 129, 160, 257):   # iteration of one key (prefetch); dK/dV grids of 1, 2, 3 workgroups
            cs.append(_case(f"shape-{L}x{S}", L, S))
    for D in range(4, 49, 4):
        cs.append(_case(f"headdim-{D}", 33, 45, D=D))
    cs.append(_case("xcd-8", 70, 45, N=2, H=4))          # grid 3 x 8: the XCD mapping on ragged tiles
    cs.append(_case("xcd-16", 70, 45, N=2, H=8))
    cs.append(_case("xcd-6", 70, 45, N=2, H=3))          # the plain reading
    for lay, L, S in (("contig", 33, 45), ("pitch4", 33, 45), ("self", 33, 33), ("cross", 33, 45), ("own", 33, 45)):
        cs.append(_case(f"layout-{lay}", L, S, N=2, H=2, layout=lay))
    cs.append(_case("layout-pitch4-n1", 65, 129, layout="pitch4"))
    cs.append(_case("logits-big", 33, 129, kind="big"))
    cs.append(_case("logits-inc", 33, 129, kind="inc"))
    cs.append(_case("logits-inc-257", 33, 257, kind="inc"))
    cs.append(_case("logits-dec", 33, 129, kind="dec"))
    cs.append(_case("logits-last-45", 33, 45, kind="last"))
    cs.append(_case("logits-last-129", 33, 129, kind="last"))
    cs.append(_case("logits-equal", 33, 129, kind="equal"))
    cs.append(_case("logits-neg80", 33, 129, kind="neg80"))
    for p in (0.1, 0.5):
        for L, S in ((70, 45), (33, 130), (32, 129)):
            cs.append(_case(f"dropout-{p}-{L}x{S}", L, S, N=2, p=p))
            cs.append(_case(f"dropout-{p}-{L}x{S}-packed", L, S, N=2, p=p, layout="cross"))
        cs.append(_case(f"dropout-{p}-self", 70, 70, N=2, p=p, layout="self"))
    cs.append(_case("dropout-0.5-onekey", 33, 1, N=2, p=0.5))
    h = torch.float16
    for L, S in ((33, 45), (65, 129), (32, 257)):
        cs.append(_case(f"half-shape-{L}x{S}", L, S, dtype=h))
    for D in (4, 36, 48):
        cs.append(_case(f"half-headdim-{D}", 33, 45, D=D, dtype=h, layout="pitch4"))
    cs.append(_case("half-dropout", 33, 130, N=2, p=0.1, dtype=h, layout="cross", do_scale=1024.0))
    cs.append(_case("half-big", 33, 129, kind="big", dtype=h))             # dO unscaled: c |dS| |k| would near 65504
    cs.append(_case("half-doscale", 33, 45, dtype=h, do_scale=1024.0))     # upstream gradient times 2^10 (a GradScaler's)
    cs.append(_case("half-doscale-self", 65, 65, N=2, dtype=h, do_scale=1024.0, layout="self"))
    return cs


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def case_inputs(case):
    seed = CASE_IDS.index(case["id"])
    return make_inputs(case["L"], case["S"], case["N"], case["H"], case["D"], case["kind"], seed, case["dtype"],
                       case["do_scale"])
