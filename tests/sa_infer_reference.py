"""Float64 reference of the inference set-abstraction stage (csrc/sa_infer.hip, include/omnipq_sa.h: omnipq_sa_infer), the
elementwise error bound its arithmetic allows, a CPU emulation of that arithmetic with eight mutants, and the case table both
suites walk (tests/test_sa_infer_reference.py on the CPU, tests/test_gpu_sa_infer.py on the GPU).  Plain torch on the CPU.

    x0[p]    = [feat_pm[b][idx[p]] | (xyz[b][idx[p]] - new_xyz[b][j]) * inv_radius | 0 .. kpad)        e16
    x_{l+1}  = relu(a_l .* (W_l x_l) + b_l),  a = gamma / sqrt(running_var + eps),  b = beta - running_mean a
    out      = max over the ball's S rows of the last layer                                          f32, and its e16 rounding

The reference is evaluated in float64 from the operands the kernel reads: the e16 features, the e16 PREPARED weights (layer 0:
[C][kpad] with the columns [features(cin) | xyz(3) | 0], what omnipq_prep_weight leaves with rot = 3) and the relative
coordinates computed in f32 (subtract, then multiply) and rounded to e16, exactly as omnipq_sa_gather stores them.  Its a, b
are formed in float64 from the f32 vectors.

Bound, per element, propagated through the chain.  u = unit_roundoff, eta = abs_roundoff, MARGIN = 1.5 as in gemm_reference.py;
K_l = the contraction length; |.| elementwise, |W| |x| the product of the absolute values (float64):

    E_0     = 0                                                       (the kernel reads the reference's own operands)
    E_{l+1} = |a_l| (|W_l| E_l) + MARGIN (u |x_{l+1}| + K_l 2^-24 |a_l| (|W_l| |x_l|) + F_l) + eta
    F_l     = F_OPS 2^-24 (|a_l| (|W_l| |x_l|) + |beta_l| + |running_mean_l| |a_l|)

The first term carries the layer's input error through the (linear) contraction and the affine; ReLU and max are 1-Lipschitz,
so nothing else is needed for them.  u |x_{l+1}| is the ONE rounding of a hidden activation to e16; K 2^-24 |a| (|W| |x|) bounds
the f32 accumulation in any order (products of two e16 values are exact in f32).  F is the f32 arithmetic of forming a, b and of
the affine on the accumulator, operation by operation: a takes three roundings (var + eps, sqrt, divide), so |a~ - a| <= 3 eps
|a|; b~ = beta - running_mean a~ adds one for the product and one for the difference, |b~ - b| <= 4 eps |running_mean a| +
eps (|beta| + |running_mean a|); a~ acc + b~ adds one for the product and one for the sum.  Together, to first order,
    5 eps |a| |W x| + 6 eps (|beta| + |running_mean| |a|)   <=   F with F_OPS = 6  (|W x| <= |W| |x|; the sum |beta| +
|running_mean| |a| stands for |b| because b may cancel while its error does not).  eps = 2^-24.
The pooled output's bound is the maximum of the last layer's E over the ball's rows; the last layer is not rounded, so its E
has no u term (and no eta): out_f32 is compared against that, out_pm gets u |out| + eta on top.

MARGIN is for what is not modelled (second-order terms); it is not tuned to any result.
"""
import functools
import math

import torch

from gemm_reference import F32_EPS, MARGIN, abs_roundoff, lib_name, unit_roundoff

F_OPS = 6
DTYPES = (torch.bfloat16, torch.float16)


def tile_rows(S):
    """rows of a workgroup's tile (csrc/sa_infer.hip): 64, 128 when a ball has 128 rows"""
    return 128 if S == 128 else 64


def kpad_of(cin):
    return (cin + 3 + 31) // 32 * 32


# ---- the cases --------------------------------------------------------------------------------------------------------------
# The smallest shapes at which the kernel can still go wrong.  idx is drawn uniformly in [0, N) unless the case says otherwise:
# valid input (the kernel only gathers), and every row is distinct, so a dropped row shows.

def _cases():
    table = [
        # id, (B, N, M, S), cin, widths, kind
        ("partial-tile", (2, 512, 13, 16), 0, (32, 32, 64), "uniform"),
        ("sa1-like", (1, 512, 8, 64), 0, (128, 128, 256), "uniform"),
        ("features", (2, 512, 9, 32), 128, (128, 128, 256), "uniform"),
        ("odd-widths-kpad320", (1, 256, 10, 16), 288, (288, 288, 288), "uniform"),
        ("kpad544", (1, 256, 6, 16), 512, (256, 256, 512), "uniform"),
        ("one-ball-per-tile", (1, 256, 5, 128), 8, (32, 64), "uniform"),
        ("one-layer", (1, 128, 4, 16), 16, (64,), "uniform"),
        # idx from the oracle's ball query on a synthetic room cloud: padded balls hold copies of their first neighbour
        ("ball-query", (2, 2048, 12, 16), 32, (64, 64, 96), "ball_query"),
        # negative gamma in every layer, running variances spread over 1e-3 .. 10
        ("negative-gamma", (1, 256, 7, 16), 32, (64, 32, 96), "negative_gamma"),
    ]
    out = []
    for name, shape, cin, widths, kind in table:
        for dt in DTYPES:
            out.append(dict(id=f"{lib_name(dt)}-{name}", name=name, shape=shape, cin=cin, widths=widths, kind=kind, dtype=dt))
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
CASE_NAMES = sorted({c["name"] for c in CASES})
RADIUS = 0.4                                             # inv_radius = 2.5: the `inv_radius dropped` mutant needs it off 1
PROBES = 4                                               # channels 0 .. 3 of every layer, see make_inputs
PROBE_GAIN = (1.3125, -1.1875, 1.4375, -1.5625)          # five significant bits: exact in both element types
DEAD_EVERY = 8                                           # channels c % 8 == 5 of the last layer are negative in every row


def case_of(id):
    return CASES[CASE_IDS.index(id)]


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def _gather_rows(xyz, new_xyz, idx, feat, cin, kpad, inv_radius, dt, centre_shift=0, scale=True):
    """the grouped rows as omnipq_sa_gather stores them, e16 [P][kpad].  centre_shift / scale: the mutants' defects."""
    B, M, S = idx.shape
    b = torch.arange(B).view(B, 1, 1).expand(B, M, S)
    pts = xyz[b, idx.long()]                                                     # (B, M, S, 3) f32
    cen = new_xyz.reshape(B * M, 3)
    if centre_shift:
        cen = cen.roll(-centre_shift, dims=0)
    rel = pts - cen.view(B, M, 1, 3)                                             # f32: subtract ...
    if scale:
        rel = rel * torch.tensor(inv_radius, dtype=torch.float32)                # ... then multiply
    X = torch.zeros((B * M * S, kpad), dtype=dt)
    if cin:
        X[:, :cin] = feat[b, idx.long()].reshape(B * M * S, cin)
    X[:, cin:cin + 3] = rel.reshape(-1, 3).to(dt)
    return X


def make_inputs(case):
    """-> dict(xyz, new_xyz (f32), idx (int32), feat (e16 [B][N][cin] or None), inv_radius, layers), layers = list of
    dict(W (e16 [C][K], prepared), gamma, beta, mean, var (f32 [C]), eps).

    The BatchNorm vectors are CALIBRATED like those of a trained network: running_mean is close to the mean of the layer's
    pre-BatchNorm output over the case's rows and running_var to its variance (the weight rows are scaled to a target spread
    per channel), so every layer's activations are of order one and a x + b cancels -- the situation in which a second
    rounding of the pre-BatchNorm value (the stored route's Y) is visible.
    Probe channels 0 .. PROBES - 1: in layer 0 a probe reads ONE operand column through a five-bit weight -- the first two
    feature column 0, whose values sit near 100, the other two the x coordinate; without features all four read the x
    coordinate, and the centres are displaced by -40 along x so that it sits near 100 (valid input: the kernel only subtracts).
    The point every ball's LAST row reads (uniform idx; in the ball-query case: the last row of one full ball) holds the
    largest value of that column, so the row decides the probes' maxima.  In every later layer a probe copies its own channel (one weight of +-1, gamma =
    +-1, beta = 0, mean = 0, var = 1).  A probe's value reaches the output without being mixed with other channels, so a defect
    in one hidden activation is not averaged away by the contractions behind it.
    Dead channels c % 8 == 5 of the last layer: beta = -8 |gamma| with unit spread, negative in every row (the pooled value
    is relu's zero)."""
    B, N, M, S = case["shape"]
    cin, widths, dt, kind = case["cin"], case["widths"], case["dtype"], case["kind"]
    kpad = kpad_of(cin)
    gen = torch.Generator().manual_seed(7100 + CASE_NAMES.index(case["name"]))
    if kind == "ball_query":
        import synth
        from oracle import oracle_ext
        xyz = synth.make_clouds(61, B, N, kind="room")[..., :3].contiguous()
        pick = torch.stack([torch.randperm(N, generator=gen)[:M] for _ in range(B)])
        new_xyz = xyz[torch.arange(B).view(B, 1), pick].contiguous()
        idx = oracle_ext.ball_query(new_xyz, xyz, RADIUS, S).to(torch.int32)
        filled = (idx != idx[:, :, :1]).sum(dim=2) + 1
        assert int(filled.min()) < S and int(filled.max()) == S, "the case needs padded balls and full ones"
        full = (filled == S).nonzero()[0]
        special = [(int(full[0]), int(idx[full[0], full[1], S - 1]))]            # the last row of one full ball
    else:
        xyz = torch.rand((B, N, 3), generator=gen)
        new_xyz = torch.rand((B, M, 3), generator=gen)
        if cin == 0:
            new_xyz[..., 0] -= 40.0                      # the probes' operand: x coordinates near 40 * inv_radius = 100
        idx = torch.randint(0, N, (B, M, S), generator=gen).to(torch.int32)
        idx[:, :, S - 1] = N - 1                         # every ball's LAST row is the point that tops the probes
        special = [(b, N - 1) for b in range(B)]
        if cin == 0:
            xyz[:, N - 1, 0] = 1.6
    feat = None
    if cin:
        feat = torch.randn((B, N, cin), generator=gen)
        feat[..., 0] = 100.0 + 1.5 * torch.randn((B, N), generator=gen)
        for b, q in special:
            feat[b, q, 0] = 112.0
        feat = feat.to(dt)
    inv_radius = 1.0 / RADIUS
    negative = kind == "negative_gamma"
    x = _gather_rows(xyz, new_xyz, idx, feat, cin, kpad, inv_radius, dt).double()
    layers = []
    for l, C in enumerate(widths):
        K = kpad if l == 0 else widths[l - 1]
        last = l == len(widths) - 1
        W = torch.randn((C, K), generator=gen) / math.sqrt(K)
        if l == 0:
            W[:, cin + 3:] = 0.0
            if cin:
                W[:, 0] *= 0.01                          # the column near 100 feeds the probes; the others see little of it
        sign = -1.0 if negative else 1.0
        gamma = sign * (0.5 + torch.rand(C, generator=gen))
        beta = 0.5 * torch.randn(C, generator=gen)
        if negative:
            target = torch.exp(torch.empty(C).uniform_(math.log(1e-3), math.log(10.0), generator=gen)).sqrt()
        else:
            target = 0.7 + 0.7 * torch.rand(C, generator=gen)
        probe = torch.arange(C) < PROBES
        W[:PROBES] = 0.0
        if l == 0:
            W[:PROBES // 2, 0] = torch.tensor(PROBE_GAIN[:PROBES // 2])          # feature 0 (cin == 0: the x coordinate)
            W[PROBES // 2:PROBES, cin] = torch.tensor(PROBE_GAIN[PROBES // 2:])      # the x coordinate
        else:
            W[torch.arange(PROBES), torch.arange(PROBES)] = sign
        acc = x @ W.double().T
        std = acc.std(dim=0).clamp_min(1e-6)
        scale = torch.where(probe, torch.ones(C, dtype=torch.float64), target.double() / std)
        W = (W.double() * scale.view(C, 1)).float().to(dt)
        acc = x @ W.double().T
        mean = (acc.mean(dim=0) + 0.1 * acc.std(dim=0) * torch.randn(C, generator=gen).double()).float()
        var = (acc.var(dim=0) * (0.8 + 0.4 * torch.rand(C, generator=gen).double())).float().clamp_min(1e-6)
        if l > 0:                                        # a probe copies its channel
            gamma[:PROBES], beta[:PROBES], mean[:PROBES], var[:PROBES] = sign, 0.0, 0.0, 1.0
        if last:
            dead = torch.arange(C) % DEAD_EVERY == 5
            beta[dead] = -8.0 * gamma[dead].abs()
        eps = 1e-5 if l != 1 else 1e-3
        lay = dict(W=W, gamma=gamma.float(), beta=beta.float(), mean=mean, var=var, eps=eps)
        layers.append(lay)
        a, b = _affine64(lay)
        x = torch.relu(acc * a + b)
    return dict(xyz=xyz, new_xyz=new_xyz, idx=idx, feat=feat, inv_radius=inv_radius, layers=layers)


def _affine64(lay):
    a = lay["gamma"].double() / torch.sqrt(lay["var"].double() + float(torch.tensor(lay["eps"], dtype=torch.float32)))
    return a, lay["beta"].double() - lay["mean"].double() * a


# ---- reference and bounds ---------------------------------------------------------------------------------------------------

def reference(inp, shape, cin, dtype):
    """-> dict(out (float64 [B M][C]), bound_f32, bound_pm): the pooled output and its elementwise bounds"""
    B, N, M, S = shape
    u, eta = unit_roundoff(dtype), abs_roundoff(dtype)
    kpad = inp["layers"][0]["W"].shape[1]
    x = _gather_rows(inp["xyz"], inp["new_xyz"], inp["idx"], inp["feat"], cin, kpad, inp["inv_radius"], dtype).double()
    E = torch.zeros_like(x)
    L = len(inp["layers"])
    for l, lay in enumerate(inp["layers"]):
        W = lay["W"].double()
        K = W.shape[1]
        a, b = _affine64(lay)
        z, S_abs = x @ W.T, x.abs() @ W.abs().T
        nxt = torch.relu(z * a + b)
        F = F_OPS * F32_EPS * (a.abs() * S_abs + lay["beta"].double().abs() + lay["mean"].double().abs() * a.abs())
        carried = a.abs() * (E @ W.abs().T)
        if l < L - 1:
            E = carried + MARGIN * (u * nxt.abs() + K * F32_EPS * a.abs() * S_abs + F) + eta
        else:
            E = carried + MARGIN * (K * F32_EPS * a.abs() * S_abs + F)
        x = nxt
    C = x.shape[1]
    out = x.view(B * M, S, C).max(dim=1).values
    bound = E.view(B * M, S, C).max(dim=1).values
    return dict(out=out, bound_f32=bound, bound_pm=bound + u * out.abs() + eta)


def ratios(got_f32, got_pm, ref):
    """-> {output: (largest error / bound, elements outside)}; a non-finite element counts as outside"""
    out = {}
    for name, got, bnd in (("out_f32", got_f32, ref["bound_f32"]), ("out_pm", got_pm, ref["bound_pm"])):
        err = (got.double() - ref["out"]).abs()
        inside = err <= bnd
        r = err / bnd
        r = torch.where((bnd == 0) & (err == 0), torch.zeros_like(r), r)
        r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
        out[name] = (float(r.max()), int((~inside).sum()))
    return out


def outside(rat):
    return {n: r for n, r in rat.items() if r[1]}


def fmt(rat):
    return " ".join(f"{n}={r[0]:.3f}" for n, r in rat.items())


# ---- the kernel's arithmetic on the CPU -------------------------------------------------------------------------------------

MUTANTS = ("pool_s_minus_1", "no_last_relu", "unrotated_w0", "next_layers_b", "neighbour_centre", "no_inv_radius",
           "round_twice", "partial_tile_ball0")


def applies(mutant, case):
    """does the defect change anything on this case's shape?"""
    B, N, M, S = case["shape"]
    L = len(case["widths"])
    if mutant == "unrotated_w0":
        return case["cin"] > 0                           # without features the rotation is the identity
    if mutant in ("next_layers_b", "round_twice"):
        return L >= 2                                    # needs a hidden layer
    if mutant == "partial_tile_ball0":
        return (B * M * S) % tile_rows(S) != 0
    return True


def emulate(inp, shape, cin, dtype, mutant=None):
    """f32 accumulation, a / b formed in f32, the affine and ReLU on the f32 accumulator, ONE e16 rounding per hidden
    activation, the pooled maximum in f32.  -> (out_f32 [B M][C], out_pm e16).  mutant: one of MUTANTS --
      pool_s_minus_1      the ball maximum over S - 1 rows
      no_last_relu        no ReLU on the last layer
      unrotated_w0        layer 0's weight columns as the parameter has them ([xyz | features]) against rows [features | xyz]
      next_layers_b       layer l + 1's b used in layer l (hidden layers)
      neighbour_centre    the next ball's centre
      no_inv_radius       the relative coordinates not scaled
      round_twice         a hidden activation through Y in e16 and then the affine, as the stored route computes it
      partial_tile_ball0  the rows a partial last tile lacks read as ball 0's, and the last ball's maximum runs over them"""
    assert mutant is None or mutant in MUTANTS
    B, N, M, S = shape
    f32 = torch.float32
    kpad = inp["layers"][0]["W"].shape[1]
    x = _gather_rows(inp["xyz"], inp["new_xyz"], inp["idx"], inp["feat"], cin, kpad, inp["inv_radius"], dtype,
                     centre_shift=1 if mutant == "neighbour_centre" else 0, scale=mutant != "no_inv_radius").to(f32)
    L = len(inp["layers"])
    ab = []
    for lay in inp["layers"]:
        a = lay["gamma"] / torch.sqrt(lay["var"] + torch.tensor(lay["eps"], dtype=f32))
        ab.append((a, lay["beta"] - lay["mean"] * a))
    for l, lay in enumerate(inp["layers"]):
        W = lay["W"].to(f32)
        if l == 0 and mutant == "unrotated_w0":
            W = torch.cat([W[:, cin:cin + 3], W[:, :cin], W[:, cin + 3:]], dim=1)
        a, b = ab[l]
        if mutant == "next_layers_b" and l < L - 1:
            nb = ab[l + 1][1]
            b = nb[torch.arange(a.numel()) % nb.numel()]
        acc = x @ W.T
        last = l == L - 1
        if mutant == "round_twice" and not last:
            acc = acc.to(dtype).to(f32)
        y = a * acc + b
        if not (last and mutant == "no_last_relu"):
            y = torch.relu(y)
        x = y if last else y.to(dtype).to(f32)
    C = x.shape[1]
    rows = x.view(B * M, S, C)
    out = (rows[:, :S - 1] if mutant == "pool_s_minus_1" else rows).max(dim=1).values
    if mutant == "partial_tile_ball0":
        out = out.clone()
        out[-1] = torch.maximum(out[-1], out[0])
    return out, out.to(dtype)


@functools.lru_cache(maxsize=None)
def case_data(id):
    """-> (inputs, reference with bounds) of the case: computed once, shared, not to be modified"""
    case = case_of(id)
    inp = make_inputs(case)
    return inp, reference(inp, case["shape"], case["cin"], case["dtype"])
