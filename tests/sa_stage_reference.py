"""Float64 reference of the streaming kernels of the training set-abstraction stage (csrc/sa_stage.hip), the elementwise error
bounds their roundings allow, a CPU emulation of the kernels' arithmetic with mutants, and the case tables both suites walk.
Plain torch / numpy on the CPU, in the conventions of tests/decoder_reference.py (MARGIN, U32, unit_roundoff / abs_roundoff,
ratios).

The reference is evaluated in float64 from the tensors a kernel reads: e16 operands (the library's 16-bit type) as stored,
f32 vectors as stored, C scalars as the f32 / f64 the ABI carries.  p = (bm, t) is row t of ball bm, P rows in all.

    gather       X[p] = [feat[b][idx[p]] | e16((xyz[b][idx[p]] - centre[bm]) inv_r) | 0 ...], kpad columns
    statistics   sums = [sum_p y | sum_p y^2]  (the _z entries ADD to what the buffer holds)
    finalize     mu = s1 / cnt, var = max(s2 / cnt - mu^2, 0), invstd = (var + eps)^-1/2, a = gamma invstd, b = beta - mu a
                 running_mean = (1 - mom) rm + mom (mu + conv_bias)
                 running_var  = (1 - mom) rv + mom var cnt / (cnt - 1)      (var itself when cnt <= 1)
    normalise    x = relu(a y + b)
    pool         out = max_t relu(a y + b), arg = the first row attaining it (row 0 when everything is clamped)
    pool_select  y* = the ball's maximum where a >= 0, its minimum where a < 0; ysel = y*; out = relu(a y* + b);
                 arg = the first row attaining y*, 0 where out == 0
    pool bwd     dz = g_out at row arg where out_pm > 0, else 0;  S = sum dz, T = sum dz yhat, yhat = (y - mean) invstd
                 dY = a (dz - S / Ptot - yhat T / Ptot)
    dense bwd    dz = dX [a y + b > 0], the same S, T, dY
    scatter      dfeat[b][k] = sum_{p: idx[p] = k} dX[p][:cin],  dxyz[b][k] = inv_r sum dX[p][cin:cin+3]
                 dcentre[bm] = -inv_r sum_t dX[(bm, t)][cin:cin+3]
    scatter_rows_csr   the same with dfeat from dY [P][C] and the coordinate sums from dXr [P][8], columns 0..2

Decisions are exact.  The kernels gate with ONE fused multiply-add, fmaf(a, y, b) > 0, and pool with a strict > on that f32
number.  For |a| in [2^-3, 2^2] or 0, |y| in [2^-6, 2^3] or 0, |b| in [2^-6, 2^2] or 0 the sum a y + b is exact in float64
(`in_exact_ranges`, asserted by every case builder; tests/test_sa_stage_reference.py re-checks samples against
fractions.Fraction), so its sign, its f32 rounding, the first-maximum row and e16(out) > 0 follow exactly from float64: no
element is ever excluded from a comparison.  The "mean 8, spread 2^-4" channel leaves that range of y, so it appears where no
gate reads y (the forward statistics and finalize); every kernel behind a gate carries a "mean 6, spread 2^-4" channel
instead (|mean| / sigma = 96, inside the range), which is where the fused apply kernel's cancellation shows.

Bounds.  u32 = 2^-24 per f32 operation, u / eta per e16 store, all times MARGIN = 1.5.  A statistics kernel sums a column
as: a lane's chain of L = ceil(rows / (grid rpb)) terms, the fold of the block's rpb row groups, then float64 -- an element
passes through at most n = (L - 1) + (min(rpb, rows) - 1) f32 additions (`chain`; rpb / grid are rows_per_block /
stats_grid of sa_stage.hip restated, the _sel entries cap the grid at 128).

    sum y        e_s1 = n u32 sum|y|               sum y^2   e_s2 = (n + 1) u32 sum y^2      (+ 2^-52 per f64 atomic)
    mu           e_mu = e_s1 / cnt + 2^-52 |mu|
    var          e_var = e_s2 / cnt + 2 |mu| e_mu + 2^-51 (s2 / cnt + mu^2)       the cancellation s2 / cnt - mu^2
    invstd       e_is = invstd e_var / (2 (var + eps)) + u32 invstd               f64 sqrt and division, one f32 rounding
    a            e_a = |gamma| e_is + u32 |a|
    b            e_b = |mu| e_a + |a| (e_mu + u32 |mu|) + u32 (|mu a| + |b|)
    mean         e_mu + u32 |mu|
    running_mean u32 (2 |(1 - mom) rm| + |mu + bias| mom + |mom (mu + bias)| + |result|) + mom (e_mu + u32 |mu|)
    running_var  u32 (2 |(1 - mom) rv| + 2 mom |unbiased| + |result|) + mom e_var cnt / (cnt - 1)
    normalise    (u32 + u) |x| + eta;  pool out_f32: u32 |out|  (the only rounding of an exact number)
    yhat         e_yh = 2 u32 |yhat|
    S, T         e_S = n u32 sum|dz|,  e_T = sum|dz| e_yh + (n + 1) u32 sum|dz yhat|
    pooled dY    u32 (|a dz| + 2 |a S/Pt| + |a dz - a S/Pt| + 5 |a yhat T/Pt| + |dY|) + |a| e_S / Pt + |a yhat| e_T / Pt
                 + u |dY| + eta
    dense dY     (omnipq_bn_bwd_apply)  |a| u32 (|S/Pt| + |dz - S/Pt| + 4 |yhat T/Pt| + |dz - S/Pt - yhat T/Pt|) + u32 |dY|
                 + the e_S, e_T, u, eta terms above
    fused dY     (omnipq_bn_bwd_apply_fused: dY = a dz + t2 y + t3, t2 = -a invstd T/Pt, t3 = a (invstd T/Pt mean - S/Pt))
                 u32 (3 |t2 y| + 4 |a invstd T/Pt mean| + 3 |a S/Pt| + 2 |t3| + |t2 y + t3| + |dY|) + the same tail:
                 |t2 y| and |a invstd T/Pt mean| do not cancel in the bound as they do in the value
    scatter      atomics: (k - 1) u32 sum|terms| for a bucket of k (+ u32 per term scaled by inv_r); CSR: f64 sums, one or
                 two f32 roundings; the centre gradient: (s - 1) u32 sum|d| inv_r + u32 |result|

Bit equality where there is no arithmetic or one defined rounding: gather's feature columns and pad zeros, arg, ysel,
out_pm == e16(out_f32), out_f32 itself on the cases inside the exact ranges (one rounding of an exact number), the f32 copies
of the totals (omnipq_sums_to_f32, gb_out, dbeta_dgamma), and the hot words e16(f32(a dz)) << 16 | arg.
"""
from fractions import Fraction

import torch

from decoder_reference import MARGIN, U32, abs_roundoff, as_f32, fmt, outside, ratios, unit_roundoff  # noqa: F401

F32, F64 = torch.float32, torch.float64
U64 = 2.0 ** -52
EPS = 1e-5
INV_R = as_f32(1.0 / 0.3)
WIDTHS = (16, 24, 128, 288, 640)


# ---- the launch geometry of sa_stage.hip, restated ------------------------------------------------------------------------

def rows_per_block(C):
    return min(16, 256 // (C // 8))


def stats_grid(rows, C):
    rpb = rows_per_block(C)
    blocks = -(-rows // rpb)
    if blocks > 512:
        per_lane = min(32, -(-blocks // 512))
        blocks = -(-rows // (rpb * per_lane))
    return max(1, min(blocks, 1024))


def chain(rows, C, sel=False):
    """-> (grid, rpb, L, n): workgroups, row lanes per workgroup, rows on the longest lane, f32 additions on the longest path"""
    rpb = rows_per_block(C)
    grid = stats_grid(rows, C)
    if sel:
        grid = min(grid, 128)
    L = max(1, -(-rows // (grid * rpb)))
    return grid, rpb, L, (L - 1) + (min(rpb, max(rows, 1)) - 1)


def sel_step(C):
    return 128 * rows_per_block(C)


# ---- exactness of the gate ------------------------------------------------------------------------------------------------

def _in(v, lo, hi):
    v = v.double().abs()
    return bool(((v == 0) | ((v >= 2.0 ** lo) & (v <= 2.0 ** hi))).all())


def in_exact_ranges(a, b, y):
    return _in(a, -3, 2) and _in(b, -6, 2) and _in(y, -6, 3)


def pre(a, b, y):
    """a y + b in float64 (exact inside the ranges), y (..., C)"""
    return a.double() * y.double() + b.double()


def relu32(z):
    """float64 pre-activations -> the f32 number max(fmaf(a, y, b), 0) the kernels hold; whatever is not positive is +0"""
    z = z.to(F32)
    return torch.where(z > 0, z, torch.zeros((), dtype=F32))


def fraction_mismatches(a, b, y, samples=200, seed=0):
    """how many of `samples` (row, channel) pairs have float64 a y + b different from the rational number"""
    gen = torch.Generator().manual_seed(seed)
    y2 = y.reshape(-1, y.shape[-1])
    r = torch.randint(0, y2.shape[0], (samples,), generator=gen)
    c = torch.randint(0, y2.shape[1], (samples,), generator=gen)
    z = pre(a, b, y2)
    bad = 0
    for i, j in zip(r.tolist(), c.tolist()):
        exact = Fraction(float(a[j])) * Fraction(float(y2[i, j])) + Fraction(float(b[j]))
        bad += Fraction(float(z[i, j])) != exact
    return bad


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def dy(gen, shape, lo, hi, scale=1.0):
    """signed values with magnitude clamped into [2^lo, 2^hi]"""
    v = torch.randn(shape, generator=gen) * scale
    return torch.sign(v + (v == 0)) * v.abs().clamp(2.0 ** lo, 2.0 ** hi)


def ab_vectors(gen, C):
    """a: positive, negative and zero; b likewise; channel 3: a = 1/2, b = -1 (y = 2 cancels exactly); channel 4: b = 0"""
    a, b = dy(gen, (C,), -3, 2), dy(gen, (C,), -6, 2, 0.5)
    a[1::5] = 0.0
    b[2::7] = 0.0
    a[3], b[3], b[4] = 0.5, -1.0, 0.0
    a[5] = a[5].abs()
    return a, b


def y_rows(gen, rows, C, dtype, free=False):
    """pre-BatchNorm activations: channel 3 carries y = 2 and channel 4 y = 0 on a third of the rows (exactly zero
    pre-activations with ab_vectors), channel 5 has mean 6 and spread 2^-4, channel 6 is constant, and with `free` (no gate
    reads y) channel 7 has mean 8 and spread 2^-4"""
    y = dy(gen, (rows, C), -6, 3)
    y[torch.rand((rows, C), generator=gen) < 0.05] = 0.0
    hit = torch.rand(rows, generator=gen) < 0.34
    y[hit, 3], y[hit, 4] = 2.0, 0.0
    y[:, 5] = (6.0 + 2.0 ** -4 * torch.randn(rows, generator=gen)).clamp(4.0, 8.0)
    y[:, 6] = 1.25
    if free:
        y[:, 7] = 8.0 + 2.0 ** -4 * torch.randn(rows, generator=gen)
    return y.to(dtype)


def moments(y):
    """per-channel mean and invstd of y as f32 vectors (what a finalize would have stored, give or take)"""
    yd = y.double().reshape(-1, y.shape[-1])
    mu = yd.mean(dim=0)
    var = ((yd - mu) ** 2).mean(dim=0)
    return mu.to(F32), ((var + EPS) ** -0.5).to(F32)


def pad_balls(gen, y, s):
    """(BM, s, C): every third ball keeps 1 + (ball % s) rows and repeats its first row behind them (exact ties)"""
    for bm in range(0, y.shape[0], 3):
        y[bm, 1 + bm % s:] = y[bm, 0]
    return y


# ---- checking -------------------------------------------------------------------------------------------------------------

def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def verdict(got, want, bnd, exact):
    """-> (ratios over the bounded outputs, names of the outputs that broke a bound or a bit equality)"""
    rat = ratios({n: g for n, g in got.items() if n in bnd}, want, bnd)
    broken = sorted(outside(rat))
    for n, e in exact.items():
        if n in got and (got[n].dtype != e.dtype or got[n].shape != e.shape or not torch.equal(bits(got[n]), bits(e))):
            broken.append(n + "(bits)")
    assert set(bnd) | set(exact) >= set(got), set(got) - set(bnd) - set(exact)
    return rat, broken


# ---- gather ---------------------------------------------------------------------------------------------------------------

def ball_indices(gen, b, n, m, s):
    """int32 (b m s): neighbours in [0, n); every other ball is padded with copies of its first neighbour"""
    idx = torch.randint(0, n, (b * m, s), generator=gen, dtype=torch.int32)
    for bm in range(0, b * m, 2):
        idx[bm, 1 + bm % s:] = idx[bm, 0]
    return idx.reshape(-1)


GATHER_CASES = [dict(id=f"gather-cin{cin}-kpad{cin + k}-s{s}", b=2, n=37, m=m, s=s, cin=cin, kpad=cin + k)
                for cin, k, m, s in ((0, 8, 5, 3), (0, 16, 3, 16), (8, 8, 7, 4), (8, 16, 2, 5), (24, 8, 3, 1), (24, 16, 9, 5))]
GATHER_CASES.append(dict(id="gather-stride", b=2, n=300, m=300, s=16, cin=8, kpad=16))     # 19 200 pieces: > one grid row


def gather_inputs(case, dtype):
    gen = torch.Generator().manual_seed(100 + GATHER_CASES.index(case))
    b, n, m, s, cin = (case[k] for k in ("b", "n", "m", "s", "cin"))
    return dict(case, xyz=torch.randn((b, n, 3), generator=gen), centre=torch.randn((b * m, 3), generator=gen),
                idx=ball_indices(gen, b, n, m, s), feat=torch.randn((b, n, cin), generator=gen).to(dtype), inv_r=INV_R)


def _src_rows(inp):
    """row of the (b n) source table every position reads"""
    P = inp["b"] * inp["m"] * inp["s"]
    scene = torch.arange(P) // (inp["m"] * inp["s"])
    return scene * inp["n"] + inp["idx"].long()


def gather_reference(inp, dtype):
    src = _src_rows(inp)
    ball = torch.arange(src.numel()) // inp["s"]
    rel = (inp["xyz"].reshape(-1, 3)[src].double() - inp["centre"][ball].double()) * inp["inv_r"]
    want = dict(rel=rel)
    bnd = dict(rel=MARGIN * ((2 * U32 + unit_roundoff(dtype)) * rel.abs() + abs_roundoff(dtype)))
    exact = dict(feat_cols=inp["feat"].reshape(inp["b"] * inp["n"], inp["cin"])[src],
                 pad_cols=torch.zeros((src.numel(), inp["kpad"] - inp["cin"] - 3), dtype=dtype))
    return want, bnd, exact


def split_gathered(X, cin):
    return dict(feat_cols=X[:, :cin].contiguous(), rel=X[:, cin:cin + 3].contiguous(), pad_cols=X[:, cin + 3:].contiguous())


def gather_emulate(inp, dtype, mutant=None):
    src = _src_rows(inp)
    ball = torch.arange(src.numel()) // inp["s"]
    d = inp["xyz"].reshape(-1, 3)[src] - inp["centre"][ball]
    if mutant == "gather_round_before_scale":
        d = d.to(dtype).to(F32)
    X = torch.zeros((src.numel(), inp["kpad"]), dtype=dtype)
    X[:, :inp["cin"]] = inp["feat"].reshape(inp["b"] * inp["n"], inp["cin"])[src]
    X[:, inp["cin"]:inp["cin"] + 3] = (d * torch.tensor(inp["inv_r"], dtype=F32)).to(dtype)
    if mutant == "pad_nonzero":
        X[-1, -1] = 2.0 ** -20
    return split_gathered(X, inp["cin"])


# ---- column statistics ----------------------------------------------------------------------------------------------------

def _row_counts(C, sel):
    rpb = rows_per_block(C)
    rows = [1, rpb - 1, rpb + 1, 512 * rpb + 1]
    if sel:
        rows += [sel_step(C) + 1, 3 * sel_step(C) + 5, 4 * sel_step(C) + 1]
    return list(dict.fromkeys(rows))                        # (rpb = 16: 512 rpb + 1 is 4 steps + 1)


STATS_SHAPES = [(C, r) for C in WIDTHS for r in _row_counts(C, False)]
SEL_SHAPES = [(C, r) for C in WIDTHS for r in _row_counts(C, True)]


def _lane_sums(terms, grid, rpb, L, mutant=None):
    """terms: list of (rows, C) f32 columns to sum plainly, or (x, w) pairs summed as fmaf(x, w, acc).  -> f64 (len, C):
    row p sits on lane (p // rpb) % grid of sub-row p % rpb in sweep p // (grid rpb); a lane adds its sweeps in turn, the block
    folds its row groups in turn (f32), the blocks meet in float64"""
    out = []
    for t in terms:
        x, w = t if isinstance(t, tuple) else (t, None)
        rows, C = x.shape
        full = L * grid * rpb
        if mutant == "stats_drop_tail" and rows > grid * rpb:
            rows = (rows // (grid * rpb)) * grid * rpb
            x, w = x[:rows], (None if w is None else w[:rows])

        def lay(v):
            return torch.cat([v, torch.zeros((full - rows, C), dtype=F32)]).reshape(L, grid, rpb, C)

        xs, ws = lay(x), (None if w is None else lay(w))
        acc = torch.zeros((grid, rpb, C), dtype=F32)
        for k in range(L):
            acc = (acc + xs[k]) if w is None else (xs[k].double() * ws[k].double() + acc.double()).to(F32)
        blk = torch.zeros((grid, C), dtype=F32)
        for r in range(rpb):
            blk = blk + acc[:, r]
        out.append(blk.double().sum(dim=0))
    return torch.stack(out)


def colstats_inputs(C, rows, dtype, sums0=False):
    gen = torch.Generator().manual_seed(200 + 7 * C + rows)
    return dict(y=y_rows(gen, rows, C, dtype, free=True), sums0=3.0 * torch.randn((2, C), generator=gen, dtype=F64) if sums0 else None)


def colstats_reference(inp):
    y = inp["y"].double()
    rows, C = y.shape
    grid, _, _, n = chain(rows, C)
    s0 = torch.zeros((2, C), dtype=F64) if inp["sums0"] is None else inp["sums0"]
    want = dict(sums=s0 + torch.stack([y.sum(dim=0), (y * y).sum(dim=0)]))
    mag = torch.stack([y.abs().sum(dim=0), (y * y).sum(dim=0)])
    e = torch.stack([n * U32 * mag[0], (n + 1) * U32 * mag[1]]) + (grid + 1) * U64 * (mag + s0.abs())
    return want, dict(sums=MARGIN * e), {}


def colstats_emulate(inp, mutant=None):
    y = inp["y"].to(F32)
    grid, rpb, L, _ = chain(*y.shape)
    s = _lane_sums([y, (y, y)], grid, rpb, L, mutant)
    return dict(sums=s if inp["sums0"] is None else s + inp["sums0"])


# ---- finalize -------------------------------------------------------------------------------------------------------------
# channels cycle through: ordinary (mu ~ N(0, 1), var ~ 1), constant (var = 0 exactly), large mean (mu = 8, var = 2^-8),
# and totals whose s2 / cnt - mu^2 is slightly NEGATIVE (what rounded partial sums of a constant channel can leave)

def _fin(id, C=24, cnt=37.0, mom=0.1, running=True, bias=True):
    return dict(id=id, C=C, cnt=cnt, mom=mom, running=running, bias=bias)


FINALIZE_CASES = [_fin("fin-plain"), _fin("fin-mom1", mom=1.0), _fin("fin-no-running", running=False),
                  _fin("fin-no-bias", bias=False), _fin("fin-cnt1", cnt=1.0), _fin("fin-cnt2", cnt=2.0),
                  _fin("fin-group", cnt=74.0), _fin("fin-C640", C=640, cnt=1537.0), _fin("fin-C16", C=16, cnt=15.0)]


def finalize_inputs(case):
    gen = torch.Generator().manual_seed(300 + [c["id"] for c in FINALIZE_CASES].index(case["id"]))
    C, cnt = case["C"], case["cnt"]
    mu = torch.randn(C, generator=gen, dtype=F64)
    var = torch.rand(C, generator=gen, dtype=F64) + 0.5
    if cnt <= 1:
        var = torch.zeros(C, dtype=F64)
    mu[1::4], var[1::4] = 1.25, 0.0
    mu[2::4], var[2::4] = 8.0, (0.0 if cnt <= 1 else 2.0 ** -8)
    mu[3::4] = 8.0
    s2 = cnt * (var + mu * mu)
    s2[3::4] = cnt * 64.0 * (1.0 - 2.0 ** -30)
    sums = torch.stack([cnt * mu, s2])                      # (fin-group: count = 2 P with doubled sums, two ranks)

    def v(scale=1.0, shift=0.0):
        return torch.randn(C, generator=gen) * scale + shift

    return dict(case, sums=sums, gamma=v(1.0), beta=v(0.5), eps=as_f32(EPS), mom=as_f32(case["mom"]),
                rm=v() if case["running"] else None, rv=v(0.2, 1.0) if case["running"] else None,
                bias=v() if case["bias"] else None)


def finalize_reference(inp, e_s1=0.0, e_s2=0.0):
    """-> (want, bounds, {}); e_s1 / e_s2: what the totals themselves may be off by (0: they are the kernel's input)"""
    s1, s2 = inp["sums"][0].double(), inp["sums"][1].double()
    cnt, eps, mom = float(inp["cnt"]), inp["eps"], inp["mom"]
    gamma, beta = inp["gamma"].double(), inp["beta"].double()
    mu = s1 / cnt
    raw = s2 / cnt - mu * mu
    var = raw.clamp(min=0.0)
    invstd = (var + eps) ** -0.5
    a = gamma * invstd
    b = beta - mu * a
    want = dict(a=a, b=b, mean=mu, invstd=invstd)
    e_mu = e_s1 / cnt + U64 * mu.abs()
    e_var = e_s2 / cnt + 2 * mu.abs() * e_mu + 2 * U64 * (s2.abs() / cnt + mu * mu)
    e_is = invstd * e_var / (2 * (var + eps)) + U32 * invstd
    e_a = gamma.abs() * e_is + U32 * a.abs()
    e_b = mu.abs() * e_a + a.abs() * (e_mu + U32 * mu.abs()) + U32 * ((mu * a).abs() + b.abs())
    bnd = dict(a=e_a, b=e_b, mean=e_mu + U32 * mu.abs(), invstd=e_is)
    if inp["rm"] is not None:
        shift = torch.zeros_like(mu) if inp["bias"] is None else inp["bias"].double()
        k = cnt / (cnt - 1) if cnt > 1 else 1.0
        old_m, old_v = (1 - mom) * inp["rm"].double(), (1 - mom) * inp["rv"].double()
        want.update(rm=old_m + mom * (mu + shift), rv=old_v + mom * var * k)
        bnd.update(rm=U32 * (2 * old_m.abs() + 2 * mom * (mu + shift).abs() + want["rm"].abs()) + mom * (e_mu + U32 * mu.abs()),
                   rv=U32 * (2 * old_v.abs() + 2 * mom * var * k + want["rv"].abs()) + mom * e_var * k)
    return want, {n: MARGIN * e for n, e in bnd.items()}, {}


FINALIZE_MUTANTS = ("rv_biased", "eps_outside", "rm_no_bias", "var_unclamped")


def finalize_emulate(inp, mutant=None):
    s1, s2 = inp["sums"][0].double(), inp["sums"][1].double()
    cnt = float(inp["cnt"])
    eps, mom = torch.tensor(inp["eps"], dtype=F32), torch.tensor(inp["mom"], dtype=F32)
    mu = s1 / cnt
    var = s2 / cnt - mu * mu
    if mutant != "var_unclamped":
        var = var.clamp(min=0.0)
    is32 = (1.0 / (var.sqrt() + eps.double()) if mutant == "eps_outside" else 1.0 / (var + eps.double()).sqrt()).to(F32)
    a = inp["gamma"] * is32
    mu32 = mu.to(F32)
    got = dict(a=a, b=inp["beta"] - mu32 * a, mean=mu32, invstd=is32)
    if inp["rm"] is not None:
        unb = var * cnt / (cnt - 1) if (cnt > 1 and mutant != "rv_biased") else var
        shift = inp["bias"] if (inp["bias"] is not None and mutant != "rm_no_bias") else torch.zeros_like(mu32)
        one = torch.tensor(1.0, dtype=F32)
        got.update(rm=(one - mom) * inp["rm"] + mom * (mu32 + shift), rv=(one - mom) * inp["rv"] + mom * unb.to(F32))
    return got


# ---- normalise and pool ---------------------------------------------------------------------------------------------------

BALL_SIZES = (1, 3, 4, 5, 16, 255)


def _pool(id, C, BM, s, gated=False):
    return dict(id=id, C=C, BM=BM, s=s, gated=gated)


def _pool_cases():
    cs = [_pool(f"pool-s{s}", 24, 7, s) for s in BALL_SIZES]
    cs += [_pool(f"pool-C{C}", C, rows_per_block(C) + 1, 5) for C in WIDTHS]
    cs += [_pool("pool-BM1", 16, 1, 4), _pool("pool-gated", 24, 5, 4, gated=True), _pool("pool-stride", 16, 2200, 3)]
    return cs


POOL_CASES = _pool_cases()


def by_id(cases, id):
    return next(c for c in cases if c["id"] == id)


def pool_inputs(case, dtype, free=False):
    """Y (BM, s, C) with padded balls, a, b; `gated`: every pre-activation <= 0 (out = 0 everywhere)"""
    gen = torch.Generator().manual_seed(400 + 13 * case["C"] + 3 * case["BM"] + case["s"])
    C, BM, s = case["C"], case["BM"], case["s"]
    a, b = ab_vectors(gen, C)
    y = pad_balls(gen, y_rows(gen, BM * s, C, dtype, free=free).reshape(BM, s, C), s)
    if case.get("gated"):
        a, b, y = a.abs(), -b.abs(), -(y.float().abs()).to(dtype)
    if not free:
        assert in_exact_ranges(a, b, y), case["id"]
    mean, invstd = moments(y)
    return dict(case, Y=y, a=a, b=b, mean=mean, invstd=invstd, g_out=torch.randn((BM, C), generator=gen))


def first_index(mask):
    """(BM, s, C) bool -> uint8 (BM, C): the first row that is true"""
    return mask.to(torch.uint8).argmax(dim=1).to(torch.uint8)


def bnrelu_reference(inp, dtype):
    x = relu32(pre(inp["a"], inp["b"], inp["Y"])).double()
    crumbs = U64 * ((inp["a"].double() * inp["Y"].double()).abs() + inp["b"].double().abs())    # a, b outside the exact ranges
    return dict(x=x), dict(x=MARGIN * ((U32 + unit_roundoff(dtype)) * x + abs_roundoff(dtype) + crumbs)), {}


def pool_reference(inp, dtype, got=None):
    """got: the device's (or the emulation's) outputs -- out_pm is held to the e16 rounding of ITS out_f32.  Inside the exact
    ranges out_f32 is the one f32 rounding of an exact number: bit equality, next to the bound"""
    x = relu32(pre(inp["a"], inp["b"], inp["Y"]))
    out = x.max(dim=1).values
    arg = first_index(x == out[:, None, :])
    exact = dict(arg=arg)
    if in_exact_ranges(inp["a"], inp["b"], inp["Y"]):
        exact["out_f32"] = out
    if got is not None:
        exact["out_pm"] = got["out_f32"].to(dtype)
    return dict(out_f32=out.double()), dict(out_f32=MARGIN * U32 * out.double()), exact


def extrema(Y):
    """-> ymax, ymin (e16, (BM, C)), amax, amin (uint8): what a ..._pool GEMM records of its stored output"""
    yd = Y.double()
    hi, lo = yd.max(dim=1).values, yd.min(dim=1).values
    amax, amin = first_index(yd == hi[:, None, :]), first_index(yd == lo[:, None, :])
    pick = lambda ix: torch.gather(Y, 1, ix.long()[:, None, :]).squeeze(1)
    return pick(amax), pick(amin), amax, amin


def pool_select_reference(inp, dtype, got=None, mutant=None):
    ymax, ymin, amax, amin = extrema(inp["Y"])
    up = (inp["a"] >= 0)[None, :] | (mutant == "select_max_for_neg_a")
    ysel, row = torch.where(up, ymax, ymin), torch.where(up, amax, amin)
    out = relu32(pre(inp["a"], inp["b"], ysel))
    exact = dict(arg=torch.where(out > 0, row, torch.zeros_like(row)), ysel=ysel)
    if in_exact_ranges(inp["a"], inp["b"], inp["Y"]):
        exact["out_f32"] = out
    if got is not None:
        exact["out_pm"] = got["out_f32"].to(dtype)
    return dict(out_f32=out.double()), dict(out_f32=MARGIN * U32 * out.double()), exact


def bnrelu_emulate(inp, dtype):
    return dict(x=relu32(pre(inp["a"], inp["b"], inp["Y"])).to(dtype))


def pool_emulate(inp, dtype, mutant=None):
    x = relu32(pre(inp["a"], inp["b"], inp["Y"]))
    out = x.max(dim=1).values
    hit = x == out[:, None, :]
    arg = first_index(hit)
    if mutant == "arg_last":
        arg = (x.shape[1] - 1 - first_index(hit.flip(1))).to(torch.uint8)
    return dict(out_f32=out, out_pm=out.to(dtype), arg=arg)


def pool_select_emulate(inp, dtype, mutant=None):
    want, _, exact = pool_select_reference(inp, dtype, mutant=mutant)
    out = want["out_f32"].to(F32)
    return dict(out_f32=out, out_pm=out.to(dtype), arg=exact["arg"], ysel=exact["ysel"])


# ---- backward: statistics ---------------------------------------------------------------------------------------------------
# kind "pool": dz = g_out at arg where out_pm > 0, y = Y at arg;  "sel": the same with y = ysel;  "dense": dz = dX [a y + b > 0]

def pooled_forward(inp, dtype, select):
    """out_pm, arg (and ysel) of the forward pass, from the reference"""
    want, _, exact = (pool_select_reference if select else pool_reference)(inp, dtype)
    fwd = dict(out_pm=want["out_f32"].to(F32).to(dtype), arg=exact["arg"])
    if select:
        fwd["ysel"] = exact["ysel"]
    return fwd


def pool_stats_inputs(C, BM, dtype, select, s=3):
    case = dict(id=f"{'sel' if select else 'pool'}-stats-C{C}-BM{BM}", C=C, BM=BM, s=s)
    inp = pool_inputs(case, dtype)
    inp.update(pooled_forward(inp, dtype, select))
    inp["y_hit"] = inp["ysel"] if select else torch.gather(inp["Y"], 1, inp["arg"].long()[:, None, :]).squeeze(1)
    return inp


def dense_inputs(C, rows, dtype):
    gen = torch.Generator().manual_seed(500 + 11 * C + rows)
    a, b = ab_vectors(gen, C)
    y = y_rows(gen, rows, C, dtype)
    assert in_exact_ranges(a, b, y), (C, rows)
    mean, invstd = moments(y)
    return dict(C=C, rows=rows, Y=y, a=a, b=b, mean=mean, invstd=invstd, dX=torch.randn((rows, C), generator=gen).to(dtype))


def dz_of(inp, kind, mutant=None):
    """-> (dz, y): float64 (rows, C) each -- the rows that carry a gradient, and their pre-activations"""
    if kind == "dense":
        z = pre(inp["a"], inp["b"], inp["Y"]).to(F32)
        g = (z >= 0) if mutant == "gate_ge" else (z > 0)
        return torch.where(g, inp["dX"].double(), torch.zeros((), dtype=F64)), inp["Y"].double()
    return torch.where(inp["out_pm"].double() > 0, inp["g_out"].double(), torch.zeros((), dtype=F64)), inp["y_hit"].double()


def bwd_stats_reference(inp, kind):
    dz, y = dz_of(inp, kind)
    yhat = (y - inp["mean"].double()) * inp["invstd"].double()
    rows, C = dz.shape
    grid, _, _, n = chain(rows, C, sel=kind == "sel")
    s0 = inp.get("sums0")
    s0 = torch.zeros((2, C), dtype=F64) if s0 is None else s0
    want = dict(sums=s0 + torch.stack([dz.sum(dim=0), (dz * yhat).sum(dim=0)]))
    m0, m1 = dz.abs().sum(dim=0), (dz * yhat).abs().sum(dim=0)
    e = torch.stack([n * U32 * m0, (dz.abs() * 2 * U32 * yhat.abs()).sum(dim=0) + (n + 1) * U32 * m1])
    return want, dict(sums=MARGIN * (e + (grid + 1) * U64 * (torch.stack([m0, m1]) + s0.abs()))), {}


BWD_STATS_MUTANTS = ("gate_ge", "T_no_invstd", "swap_ST", "stats_drop_tail")


def bwd_stats_emulate(inp, kind, mutant=None):
    dz, y = dz_of(inp, kind, mutant)
    dz, y = dz.to(F32), y.to(F32)
    yhat = y - inp["mean"]
    if mutant != "T_no_invstd":
        yhat = yhat * inp["invstd"]
    grid, rpb, L, _ = chain(*dz.shape, sel=kind == "sel")
    s = _lane_sums([dz, (dz, yhat)], grid, rpb, L, mutant)
    if mutant == "swap_ST":
        s = s.flip(0)
    return dict(sums=s if inp.get("sums0") is None else s + inp["sums0"])


def hot_words(inp, dtype):
    """int32 (BM, C): e16(f32(a dz)) << 16 | arg"""
    dz = torch.where(inp["out_pm"].double() > 0, inp["g_out"], torch.zeros((), dtype=F32))
    hi = bits((inp["a"][None, :] * dz).to(dtype)).to(torch.int32) & 0xFFFF
    return ((hi << 16) | inp["arg"].to(torch.int32)).to(torch.int32)


# ---- backward: apply ------------------------------------------------------------------------------------------------------

def exact_totals(inp, kind, scale=1.0):
    """the float64 totals [S | T] a statistics pass would hand over, times `scale` (2: two ranks with the same batch)"""
    return scale * bwd_stats_reference(inp, kind)[0]["sums"]


def apply_reference(inp, kind, sums, total, dtype, form, e_S=0.0, e_T=0.0):
    """kind "pool" (dY (BM, s, C)) or "dense"; form: "pool", "plain" (omnipq_bn_bwd_apply) or "fused".  -> want, bnd, exact"""
    a, mean, invstd = inp["a"].double(), inp["mean"].double(), inp["invstd"].double()
    if kind == "dense":
        dz, y = dz_of(inp, kind)
    else:
        y = inp["Y"].double()
        rows = torch.arange(y.shape[1])[None, :, None]
        hit = (rows == inp["arg"].long()[:, None, :]) & (inp["out_pm"].double() > 0)[:, None, :]
        dz = torch.where(hit, inp["g_out"].double()[:, None, :], torch.zeros((), dtype=F64))
    S, T = sums[0].double() / total, sums[1].double() / total
    yhat = (y - mean) * invstd
    inner = dz - S - yhat * T
    dY = a * inner
    aS, ayT = (a * S).abs(), (a * yhat * T).abs()
    if form == "pool":
        e = U32 * ((a * dz).abs() + 2 * aS + (a * dz - a * S).abs() + 5 * ayT + dY.abs())
    elif form == "plain":
        e = a.abs() * U32 * (S.abs() + (dz - S).abs() + 4 * (yhat * T).abs() + inner.abs()) + U32 * dY.abs()
    else:
        t2 = -a * invstd * T
        t3 = a * (invstd * T * mean - S)
        e = U32 * (3 * (t2 * y).abs() + 4 * (a * invstd * T * mean).abs() + 3 * aS + 2 * t3.abs() + (t2 * y + t3).abs() + dY.abs())
    e = e + a.abs() * e_S / total + (a * yhat).abs() * e_T / total + unit_roundoff(dtype) * dY.abs() + abs_roundoff(dtype)
    return dict(dY=dY), dict(dY=MARGIN * e), dict(gb=sums[:2].to(F32))


APPLY_MUTANTS = ("gate_ge", "div_by_P")


def apply_emulate(inp, kind, sums, total, dtype, form, mutant=None):
    a, mean, invstd = inp["a"], inp["mean"], inp["invstd"]
    if kind == "dense":
        dz, y = dz_of(inp, kind, mutant)
        dz, y, P = dz.to(F32), inp["Y"].to(F32), inp["Y"].shape[0]
    else:
        y = inp["Y"].to(F32)
        rows = torch.arange(y.shape[1])[None, :, None]
        hit = (rows == inp["arg"].long()[:, None, :]) & (inp["out_pm"].double() > 0)[:, None, :]
        dz, P = torch.where(hit, inp["g_out"][:, None, :], torch.zeros((), dtype=F32)), y.shape[0] * y.shape[1]
    inv = 1.0 / (float(P) if mutant == "div_by_P" else total)
    m1, m2 = (sums[0].double() * inv).to(F32), (sums[1].double() * inv).to(F32)
    if form == "pool":
        dY = a * dz - m1 * a - (y - mean) * (m2 * (a * invstd))
    elif form == "plain":
        dY = a * (dz - m1 - (y - mean) * invstd * m2)
    else:
        t2, t3 = -a * invstd * m2, a * (invstd * m2 * mean - m1)
        inner = (t2.double() * y.double() + t3.double()).to(F32)
        dY = (a.double() * dz.double() + inner.double()).to(F32)
    return dict(dY=dY.to(dtype), gb=sums[:2].to(F32))


# ---- scatter --------------------------------------------------------------------------------------------------------------
# buckets per scene: point 0 long (what is left), 1 empty, 2 one entry, 3 three, 4 four, 5 five, 6 empty

def _sc(id, cin, kpad, b=2, m=6, s=5, dfeat=True, dxyz=True):
    return dict(id=id, b=b, n=7, m=m, s=s, cin=cin, kpad=kpad, dfeat=dfeat, dxyz=dxyz)


SCATTER_CASES = [_sc(f"scatter-cin{cin}-kpad{cin + k}", cin, cin + k) for cin in (0, 8, 24) for k in (8, 16)]
SCATTER_CASES += [_sc("scatter-no-dfeat", 8, 16, dfeat=False), _sc("scatter-no-dxyz", 8, 16, dxyz=False),
                  _sc("scatter-long", 8, 16, b=1, m=30, s=16)]
ROWS_CASES = [_sc("rows-C16", 16, 16), _sc("rows-C24-no-dxyz", 24, 24, dxyz=False), _sc("rows-C128-long", 128, 128, b=1, m=30, s=16)]


def bucket_indices(gen, b, ms):
    assert ms >= 14
    one = torch.tensor([2] + [3] * 3 + [4] * 4 + [5] * 5 + [0] * (ms - 13), dtype=torch.int32)
    return torch.cat([one[torch.randperm(ms, generator=gen)] for _ in range(b)])


def host_csr(idx, b, n, ms):
    """offsets (b, n + 1), order (b, ms) int32: positions bucketed by source point, in position order (a stable sort)"""
    offsets, order = torch.zeros((b, n + 1), dtype=torch.int32), torch.zeros((b, ms), dtype=torch.int32)
    for i in range(b):
        k = idx[i * ms:(i + 1) * ms].long()
        order[i] = torch.sort(k, stable=True).indices.to(torch.int32)
        offsets[i, 1:] = torch.cumsum(torch.bincount(k, minlength=n), 0).to(torch.int32)
    return offsets, order


def scatter_inputs(case, dtype, rows_form=False):
    gen = torch.Generator().manual_seed(600 + 17 * case["cin"] + case["kpad"] + case["m"] + 1000 * rows_form)
    b, n, m, s = (case[k] for k in ("b", "n", "m", "s"))
    P = b * m * s
    inp = dict(case, idx=bucket_indices(gen, b, m * s), inv_r=INV_R)

    def wide(*shape):
        """thirteen binades of scale on top of N(0, 1): a bucket's sum does not fit 24 bits, the f32 roundings show"""
        return (torch.randn(shape, generator=gen) * 2.0 ** torch.randint(-6, 7, shape, generator=gen)).to(dtype)

    if rows_form:
        inp.update(dY=wide(P, case["cin"]), dXr=wide(P, 8))
    else:
        inp.update(dX=wide(P, case["kpad"]))
    inp["offsets"], inp["order"] = host_csr(inp["idx"], b, n, m * s)
    return inp


def scatter_reference(inp, dtype, form):
    """form: "atomic", "csr" (omnipq_sa_scatter_csr) or "rows" (omnipq_sa_scatter_rows_csr: dfeat32, dfeat16).  The NULL
    outputs of a case are left out."""
    b, n, m, s, cin, inv_r = (inp[k] for k in ("b", "n", "m", "s", "cin", "inv_r"))
    feat = (inp["dY"] if form == "rows" else inp["dX"][:, :cin]).double()
    xyz = (inp["dXr"][:, :3] if form == "rows" else inp["dX"][:, cin:cin + 3]).double()
    src = _src_rows(inp)
    count = torch.bincount(src, minlength=b * n).double()[:, None]

    def bucket(v):
        z = torch.zeros((b * n, v.shape[1]), dtype=F64)
        return z.index_add(0, src, v), z.index_add(0, src, v.abs())

    u, eta = unit_roundoff(dtype), abs_roundoff(dtype)
    want, bnd = {}, {}
    f, fm = bucket(feat)
    g, gm = bucket(xyz)
    cs, cm = xyz.reshape(b * m, s, 3).sum(dim=1), xyz.abs().reshape(b * m, s, 3).sum(dim=1)
    if form == "atomic":
        if inp["dfeat"]:
            want["dfeat"], bnd["dfeat"] = f, (count - 1).clamp(min=0) * U32 * fm
        if inp["dxyz"]:
            want["dxyz"], bnd["dxyz"] = g * inv_r, count * U32 * gm * inv_r
            want["dcentre"], bnd["dcentre"] = -cs * inv_r, s * U32 * cm * inv_r
    else:
        if form == "rows":
            want["dfeat32"], bnd["dfeat32"] = f, U32 * f.abs() + count * U64 * fm
            want["dfeat16"], bnd["dfeat16"] = f, (U32 + u) * f.abs() + eta + count * U64 * fm
        elif inp["dfeat"]:
            want["dfeat"], bnd["dfeat"] = f, U32 * f.abs() + count * U64 * fm
        if inp["dxyz"]:
            want["dxyz"], bnd["dxyz"] = g * inv_r, 2 * U32 * (g * inv_r).abs() + count * U64 * gm * inv_r
            want["dcentre"], bnd["dcentre"] = -cs * inv_r, ((s - 1) * U32 * cm + U32 * cs.abs()) * inv_r
    return want, {k: MARGIN * v for k, v in bnd.items()}, {}


SCATTER_MUTANTS = ("bucket_tail_dropped", "dcentre_plus", "dxyz_no_inv_r")


def scatter_emulate(inp, dtype, form, mutant=None):
    """the CSR forms: a float64 accumulator per bucket walked four entries a trip, then the tail; one f32 rounding (two with
    inv_r); the centre gradient is an f32 chain over the ball.  The atomic form adds f32 terms in position order."""
    b, n, m, s, cin = (inp[k] for k in ("b", "n", "m", "s", "cin"))
    ms = m * s
    inv_r = torch.tensor(inp["inv_r"], dtype=F32)
    feat = inp["dY"] if form == "rows" else inp["dX"][:, :cin]
    xyz = inp["dXr"][:, :3] if form == "rows" else inp["dX"][:, cin:cin + 3]
    got = {}
    if form == "atomic":
        src = _src_rows(inp)
        f, g = torch.zeros((b * n, cin), dtype=F32), torch.zeros((b * n, 3), dtype=F32)
        c = torch.zeros((b * m, 3), dtype=F32)
        for p in range(src.numel()):
            f[src[p]] += feat[p].to(F32)
            g[src[p]] += xyz[p].to(F32) * inv_r
            c[p // s] += -xyz[p].to(F32) * inv_r
    else:
        f, g = torch.zeros((b * n, feat.shape[1]), dtype=F64), torch.zeros((b * n, 3), dtype=F64)
        for i in range(b):
            for k in range(n):
                beg, end = int(inp["offsets"][i, k]), int(inp["offsets"][i, k + 1])
                if mutant == "bucket_tail_dropped":
                    end = beg + 4 * ((end - beg) // 4)
                rows = i * ms + inp["order"][i, beg:end].long()
                f[i * n + k], g[i * n + k] = feat[rows].double().sum(dim=0), xyz[rows].double().sum(dim=0)
        f = f.to(F32)
        g = g.to(F32) * (1.0 if mutant == "dxyz_no_inv_r" else inv_r)
        c = torch.zeros((b * m, 3), dtype=F32)
        for t in range(s):
            c = c + xyz.reshape(b * m, s, 3)[:, t].to(F32)
        c = (c if mutant == "dcentre_plus" else -c) * inv_r
    if form == "rows":
        got.update(dfeat32=f, dfeat16=f.to(dtype))
    elif inp["dfeat"]:
        got["dfeat"] = f
    if inp["dxyz"]:
        got.update(dxyz=g, dcentre=c)
    return got


# ---- the big case of omnipq_bn_bwd_apply_fused ------------------------------------------------------------------------------
BIG_P, BIG_C = 32776, 256            # 32776 * 32 pieces >= 2^20: four pieces per thread, non-temporal loads


assert BIG_P * (BIG_C // 8) >= 1 << 20 and MARGIN == 1.5
