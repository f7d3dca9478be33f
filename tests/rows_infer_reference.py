"""Float64 reference of the inference per-point stack (csrc/rows_infer.hip, include/omnipq_decoder.h: omnipq_rows_infer), the
elementwise error bound its arithmetic allows, a CPU emulation of that arithmetic with nine mutants, and the case table both
suites walk (tests/test_rows_infer_reference.py on the CPU, tests/test_gpu_rows_infer.py on the GPU).  Plain torch on the CPU.

    x_0      = [e16(x) | 0 .. kpad)                                       one rounding, what omnipq_pad_rows_e16 stores
    z_l      = W_l x_l                                                    f32 accumulation
    BatchNorm layer:   a = gamma / sqrt(running_var + eps),  b = beta - (running_mean - bias) a,  x_{l+1} = relu(a z + b)
    otherwise:         a = 1,  b = bias (or 0),  x_{l+1} = z + b, relu(.) when the layer's `relu` is set
    every x_{l+1}, the last one too, is rounded to e16 ONCE; the last one is the output [n][C_last]

The reference is evaluated in float64 from the operands the kernel reads: the input rounded to e16 (torch's .to() and the
kernel's conversion both round to nearest even), the e16 PREPARED weights ([C][K], zero rows up to the padded width and zero
columns behind the real contraction length, what omnipq_prep_weight leaves) and the f32 vectors; a, b are formed in float64.

Bound, per element, propagated through the chain.  u = unit_roundoff, eta = abs_roundoff, MARGIN = 1.5 as in gemm_reference.py;
K_l = the contraction length; |.| elementwise, |W| |x| the product of the absolute values (float64); eps = 2^-24:

    E_0     = 0                                                       (the kernel reads the reference's own operands)
    E_{l+1} = |a_l| (|W_l| E_l) + MARGIN (u |x_{l+1}| + K_l eps |a_l| (|W_l| |x_l|) + F_l) + eta
    F_l     = OPS_l eps (|a_l| (|W_l| |x_l|) + B_l)
    BatchNorm:  OPS = 7,  B = |beta| + (|running_mean| + |bias|) |a|;          otherwise:  OPS = 1,  B = |bias|

The first term carries the layer's input error through the (linear) contraction and the affine; ReLU is 1-Lipschitz.  u |x_{l+1}|
+ eta is the ONE rounding of the layer's output to e16 (the last layer is rounded once like the others); K eps |a| (|W| |x|)
bounds the f32 accumulation in any order (products of two e16 values are exact in f32).  F is the f32 arithmetic of forming a, b
and of the affine, operation by operation.  a takes three roundings (var + eps, sqrt, divide): |a~ - a| <= 3 eps |a|.  m =
running_mean - bias is one (|m~ - m| <= eps (|running_mean| + |bias|)), the product m~ a~ one more, the difference from beta one:
|b~ - b| <= 5 eps |m a| + eps (|beta| + |m a|).  a~ acc + b~ adds one for the product and one for the sum, eps (|a z| + |b|).
Together, to first order, 5 eps |a| |W x| + 7 eps (|beta| + |m| |a|) <= F with OPS = 7 (|W x| <= |W| |x|, |m| <= |running_mean|
+ |bias|; the sum |beta| + |m| |a| stands for |b| because b may cancel while its error does not).  Without BatchNorm a = 1 is
exact and z + bias is one rounding.

MARGIN is for what is not modelled (second-order terms); it is not tuned to any result.
"""
import functools
import math

import torch

from gemm_reference import F32_EPS, MARGIN, abs_roundoff, lib_name, unit_roundoff

OPS_BN, OPS_PLAIN = 7, 1
DTYPES = (torch.bfloat16, torch.float16)
LDS_LIMIT = 160 * 1024
ASSUMED_CUS = 256                                        # the CPU suite's "persistent" case; the GPU suite asks the device


def round_up(x, q):
    return (x + q - 1) // q * q


def lds_bytes(kpad, widths):
    """-> (bytes, rows of a tile) as include/omnipq_decoder.h states them: a | b of every layer (f32), buffer A = rows x
    (max(kpad, C_1) + 8), buffer B = rows x (max(C_0, C_2) + 8) e16; 64 rows where that fits 160 KiB, else 32"""
    wa = max([kpad] + list(widths[1:2]))
    wb = max([widths[0]] + list(widths[2:3]))
    for rows in (64, 32):
        total = 8 * sum(widths) + 2 * rows * (wa + 8 + wb + 8)
        if total <= LDS_LIMIT:
            return total, rows
    return -1, 0


# ---- the cases --------------------------------------------------------------------------------------------------------------
# The smallest shapes at which the kernel can still go wrong.  Layers: (output channels, kind), kind "bn" (BatchNorm + ReLU) |
# "relu" (bias + ReLU, the `act` kind at p = 0) | "plain".  rows None: 64 x 2 x (compute units) + 5, more tiles than the
# persistent grid has workgroups and a partial last one.

def _cases():
    table = [
        # id, input type (None: e16), cin, row pitch, layers, rows, options
        ("pos", torch.float32, 3, 3, ((288, "bn"), (288, "plain")), 77, {}),
        ("pos-pitch6", torch.float32, 3, 6, ((288, "bn"), (288, "plain")), 77, {}),
        ("pos6", torch.float32, 6, 6, ((288, "bn"), (288, "plain")), 64, {}),
        ("vote", None, 288, 288, ((288, "bn"), (288, "bn"), (291, "plain")), 300, {}),
        ("head", None, 288, 288, ((288, "bn"), (288, "bn"), (97, "plain")), 130, {}),
        ("fp", None, 512, 512, ((256, "bn"), (256, "bn")), 200, {"bias": False}),
        ("act", None, 96, 96, ((128, "bn"), (256, "relu"), (64, "plain")), 64, {}),
        ("one-layer", None, 32, 32, ((64, "plain"),), 33, {}),
        ("one-row", None, 32, 32, ((32, "bn"), (32, "plain")), 1, {}),
        ("persistent", None, 32, 32, ((32, "bn"), (32, "plain")), None, {}),
        # negative gamma in every BatchNorm layer, running variances spread over 1e-3 .. 10
        ("negative-gamma", None, 32, 32, ((64, "bn"), (32, "bn"), (96, "plain")), 70, {"negative": True}),
        # fits only with the 32-row tile
        ("1024-512-512", None, 1024, 1024, ((512, "bn"), (512, "bn")), 40, {"bias": False}),
    ]
    out = []
    for name, xdt, cin, ldx, layers, rows, opt in table:
        for dt in DTYPES:
            out.append(dict(id=f"{lib_name(dt)}-{name}", name=name, x_dtype=xdt or dt, cin=cin, ldx=ldx, layers=layers, rows=rows,
                            bias=opt.get("bias", True), negative=opt.get("negative", False), dtype=dt))
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
CASE_NAMES = sorted({c["name"] for c in CASES})
PROBES = 4                                               # channels 0 .. 3 of every layer, see make_inputs
PROBE_GAIN = (1.3125, -1.1875)                           # five significant bits: exact in both element types
PROBE_SMALL = (0.046875, -0.0546875)                     # 3 / 64, -7 / 128
CALIBRATION_ROWS = 256
JUNK = 1.0e4                                             # what lies between cin and the row pitch of a strided input


def case_of(id):
    return CASES[CASE_IDS.index(id)]


def rows_of(case, cus=ASSUMED_CUS):
    return case["rows"] if case["rows"] is not None else 64 * 2 * cus + 5


def widths_of(case):
    return tuple(round_up(c, 32) for c, _ in case["layers"])


def kpad_of(case):
    return round_up(case["cin"], 32)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def _round(t, dt):
    return t.to(dt).to(t.dtype)


def make_inputs(case, cus=ASSUMED_CUS):
    """-> dict(x (x_dtype [n][ldx]; columns cin .. ldx hold JUNK), layers), layers = list of dict(W (e16 [Cp][K], prepared),
    bias (f32 [Cp] or None), gamma, beta, mean, var (f32 [Cp], or None without BatchNorm), eps, relu).

    The BatchNorm vectors are CALIBRATED like those of a trained network, on CALIBRATION_ROWS rows of the input's distribution
    (the case's own rows may be one): running_mean is close to the mean of the layer's pre-BatchNorm output plus its conv bias,
    running_var to its variance (the weight rows are scaled to a target spread per channel), so every layer's activations are
    of order one and a z + b cancels -- the situation in which a second rounding of z shows.
    Input column 0 sits near 100 (1.5 wide), the others are of order one.
    Probe channels 0 .. PROBES - 1: in layer 0 a probe reads ONE input column through a short weight -- the first two read
    column 0 (a large z whose second rounding is visible after the cancellation), the other two column 1 through a weight of
    about 0.05, so that their running variance is about 2.5e-3, of the order of layer 0's eps = 1e-3 (a dropped eps is
    visible).  In every later layer a probe copies its own channel (one weight of +-1; BatchNorm: gamma = +-1, beta = 0, mean
    = 0, var = 1; bias 0).  A probe's value reaches the output without being mixed with other channels, so a defect in one
    hidden activation is not averaged away by the contractions behind it.
    Row 0 is built to be sensitive on its own (the one-row case): its column 0 is the e16 value in [104, 120] whose product with
    the first probe gain lies farthest from the e16 grid, and its column 1 is two spreads from the mean on the side that keeps
    a small-variance probe alive."""
    n, cin, ldx, dt, xdt = rows_of(case, cus), case["cin"], case["ldx"], case["dtype"], case["x_dtype"]
    kpad, L = kpad_of(case), len(case["layers"])
    gen = torch.Generator().manual_seed(9100 + CASE_NAMES.index(case["name"]))
    rows = max(n, CALIBRATION_ROWS)
    xr = torch.randn((rows, cin), generator=gen)
    xr[:, 0] = 100.0 + 1.5 * torch.randn(rows, generator=gen)
    cand = _round(torch.arange(104.0, 120.0, 0.0625), dt).unique()
    z = cand.double() * PROBE_GAIN[0]
    xr[0, 0] = cand[(z - _round(z.float(), dt).double()).abs().argmax()]
    sign = -1.0 if case["negative"] else 1.0
    xr[0, 1] = 2.0 * sign                                # probe 2 (positive weight) with gamma > 0, probe 3 with gamma < 0
    if xdt != torch.float32:
        xr = _round(xr, dt)
    x = torch.full((n, ldx), JUNK)
    x[:, :cin] = xr[:n]
    x = x.to(xdt)
    cur = torch.zeros((rows, kpad), dtype=torch.float64)
    cur[:, :cin] = _round(xr, dt).double()
    layers = []
    k_real = cin
    for l, (C, kind) in enumerate(case["layers"]):
        Cp, K = round_up(C, 32), cur.shape[1]
        W = torch.zeros((Cp, K))
        W[:C, :k_real] = torch.randn((C, k_real), generator=gen) / math.sqrt(k_real)
        if l == 0:
            W[:, 0] *= 0.01                              # the column near 100 feeds the probes; the others see little of it
        gamma = sign * (0.5 + torch.rand(Cp, generator=gen))
        beta = 0.5 * torch.randn(Cp, generator=gen)
        if case["negative"]:
            target = torch.exp(torch.empty(Cp).uniform_(math.log(1e-3), math.log(10.0), generator=gen)).sqrt()
        else:
            target = 0.7 + 0.7 * torch.rand(Cp, generator=gen)
        probe = torch.arange(Cp) < PROBES
        W[:PROBES] = 0.0
        if l == 0:
            W[0, 0], W[1, 0], W[2, 1], W[3, 1] = PROBE_GAIN + PROBE_SMALL
        else:
            W[torch.arange(PROBES), torch.arange(PROBES)] = sign if kind == "bn" else 1.0
        acc = cur @ W.double().T
        std = acc.std(dim=0).clamp_min(1e-6)
        scale = torch.where(probe | (torch.arange(Cp) >= C), torch.ones(Cp, dtype=torch.float64), target.double() / std)
        W = (W.double() * scale.view(Cp, 1)).float().to(dt)
        acc = cur @ W.double().T
        bias = None
        if case["bias"]:
            bias = 0.3 * torch.randn(Cp, generator=gen)
            if kind == "relu":
                bias = bias - acc.mean(dim=0).float()    # about half of a bias + ReLU layer's outputs alive
            if l > 0:
                bias[:PROBES] = 0.0
            bias[C:] = 0.0
        lay = dict(W=W, bias=bias, gamma=None, beta=None, mean=None, var=None, eps=1e-3 if l == 0 else 1e-5, relu=kind != "plain")
        if kind == "bn":
            assert C == Cp
            mean = (acc.mean(dim=0) + 0.1 * acc.std(dim=0) * torch.randn(Cp, generator=gen).double()).float()
            if bias is not None:
                mean = mean + bias                       # the running mean accounts for the conv bias
            var = (acc.var(dim=0) * (0.8 + 0.4 * torch.rand(Cp, generator=gen).double())).float().clamp_min(1e-6)
            if l == 0:
                gamma[:PROBES], beta[:PROBES] = sign, 0.25
            else:                                        # a probe copies its channel
                gamma[:PROBES], beta[:PROBES], mean[:PROBES], var[:PROBES] = sign, 0.0, 0.0, 1.0
            lay.update(gamma=gamma.float(), beta=beta.float(), mean=mean, var=var)
        layers.append(lay)
        a, b = _affine64(lay)
        cur = acc * a + b
        if lay["relu"]:
            cur = torch.relu(cur)
        k_real = C
    return dict(x=x, layers=layers)


def _affine64(lay):
    Cp = lay["W"].shape[0]
    bias = torch.zeros(Cp, dtype=torch.float64) if lay["bias"] is None else lay["bias"].double()
    if lay["gamma"] is None:
        return torch.ones(Cp, dtype=torch.float64), bias
    a = lay["gamma"].double() / torch.sqrt(lay["var"].double() + float(torch.tensor(lay["eps"], dtype=torch.float32)))
    return a, lay["beta"].double() - (lay["mean"].double() - bias) * a


def staged_rows(x, cin, kpad, dtype, fill=0.0):
    """the rows as the kernel stages them: e16 [n][kpad], one rounding, columns cin .. kpad zero (fill: the mutant's)"""
    X = torch.full((x.shape[0], kpad), fill, dtype=dtype)
    X[:, :cin] = x[:, :cin].to(dtype)
    return X


# ---- reference and bounds ---------------------------------------------------------------------------------------------------

def reference(inp, cin, dtype):
    """-> dict(out (float64 [n][C_last padded]), bound): the output and its elementwise bound"""
    u, eta = unit_roundoff(dtype), abs_roundoff(dtype)
    kpad = inp["layers"][0]["W"].shape[1]
    x = staged_rows(inp["x"], cin, kpad, dtype).double()
    E = torch.zeros_like(x)
    for lay in inp["layers"]:
        W = lay["W"].double()
        K = W.shape[1]
        a, b = _affine64(lay)
        z, S_abs = x @ W.T, x.abs() @ W.abs().T
        nxt = z * a + b
        if lay["relu"]:
            nxt = torch.relu(nxt)
        bias_abs = 0.0 if lay["bias"] is None else lay["bias"].double().abs()
        if lay["gamma"] is not None:
            F = OPS_BN * F32_EPS * (a.abs() * S_abs + lay["beta"].double().abs() + (lay["mean"].double().abs() + bias_abs) * a.abs())
        else:
            F = OPS_PLAIN * F32_EPS * (S_abs + bias_abs)
        E = a.abs() * (E @ W.abs().T) + MARGIN * (u * nxt.abs() + K * F32_EPS * a.abs() * S_abs + F) + eta
        x = nxt
    return dict(out=x, bound=E)


def ratios(got, ref):
    """-> {"out": (largest error / bound, elements outside)}; a non-finite element counts as outside"""
    err = (got.double() - ref["out"]).abs()
    bnd = ref["bound"]
    inside = err <= bnd
    r = err / bnd
    r = torch.where((bnd == 0) & (err == 0), torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return {"out": (float(r.max()), int((~inside).sum()))}


def outside(rat):
    return {n: r for n, r in rat.items() if r[1]}


def fmt(rat):
    return " ".join(f"{n}={r[0]:.3f}" for n, r in rat.items())


# ---- the kernel's arithmetic on the CPU -------------------------------------------------------------------------------------

MUTANTS = ("no_hidden_relu", "relu_on_plain_output", "bias_ignored_in_fold", "bias_twice_in_fold", "no_eps", "next_layers_b",
           "round_twice", "pad_columns_not_zeroed", "partial_tile_row0")
# rows never meet in this kernel (no pool, no statistic), so what a partial tile's missing rows hold cannot move any of the n
# output rows: this mutant is NOT visible to a bound on the output.  The emulation carries it to show exactly that (the CPU suite
# asserts its n rows are bit equal to the faithful ones); what the defect would break is "rows past n are never read", a
# property of the staging loop (its `p < n`) that no output shows.
INVISIBLE = ("partial_tile_row0",)


def applies(mutant, case):
    """does the defect change anything on this case's shape?"""
    kinds = [k for _, k in case["layers"]]
    L = len(kinds)
    if mutant == "no_hidden_relu":
        return L >= 2
    if mutant == "relu_on_plain_output":
        return kinds[-1] == "plain"
    if mutant in ("bias_ignored_in_fold", "bias_twice_in_fold"):
        return case["bias"] and "bn" in kinds
    if mutant == "no_eps":
        return "bn" in kinds
    if mutant in ("next_layers_b", "round_twice"):
        return L >= 2                                    # needs a hidden layer
    if mutant == "pad_columns_not_zeroed":
        return case["cin"] % 32 != 0
    if mutant == "partial_tile_row0":
        return False
    raise KeyError(mutant)


def emulate(inp, cin, dtype, mutant=None):
    """f32 accumulation, a / b formed in f32, the affine and ReLU on the f32 accumulator, ONE e16 rounding per layer.
    -> out e16 [n][C_last padded].  mutant: one of MUTANTS --
      no_hidden_relu          no ReLU on the hidden layers
      relu_on_plain_output    a ReLU on a last layer that has none
      bias_ignored_in_fold    b = beta - running_mean a: the conv bias of a BatchNorm layer dropped
      bias_twice_in_fold      b = beta - (running_mean - 2 bias) a: the conv bias added to z and folded as well
      no_eps                  a = gamma / sqrt(running_var)
      next_layers_b           layer l + 1's b used in layer l (hidden layers)
      round_twice             a hidden layer's z through e16 and then the affine, as the stored route computes it
      pad_columns_not_zeroed  input columns cin .. kpad hold what the LDS held before (NaN here: anything may be there)
      partial_tile_row0       the rows a partial last tile lacks read as row 0 (see INVISIBLE)"""
    assert mutant is None or mutant in MUTANTS
    f32 = torch.float32
    kpad = inp["layers"][0]["W"].shape[1]
    widths = tuple(lay["W"].shape[0] for lay in inp["layers"])
    n = inp["x"].shape[0]
    x = staged_rows(inp["x"], cin, kpad, dtype, fill=float("nan") if mutant == "pad_columns_not_zeroed" else 0.0).to(f32)
    if mutant == "partial_tile_row0":
        tr = lds_bytes(kpad, widths)[1]
        x = torch.cat([x, x[:1].expand(round_up(n, tr) - n, kpad)])
    L = len(inp["layers"])
    ab = []
    for lay in inp["layers"]:
        Cp = lay["W"].shape[0]
        bias = lay["bias"]
        if lay["gamma"] is None:
            ab.append((torch.ones(Cp), torch.zeros(Cp) if bias is None else bias))
            continue
        eps = torch.tensor(0.0 if mutant == "no_eps" else lay["eps"], dtype=f32)
        a = lay["gamma"] / torch.sqrt(lay["var"] + eps)
        mean = lay["mean"]
        if bias is not None and mutant != "bias_ignored_in_fold":
            mean = mean - (2.0 * bias if mutant == "bias_twice_in_fold" else bias)
        ab.append((a, lay["beta"] - mean * a))
    for l, lay in enumerate(inp["layers"]):
        W = lay["W"].to(f32)
        a, b = ab[l]
        last = l == L - 1
        if mutant == "next_layers_b" and not last:
            nb = ab[l + 1][1]
            b = nb[torch.arange(a.numel()) % nb.numel()]
        acc = x @ W.T
        if mutant == "round_twice" and not last:
            acc = acc.to(dtype).to(f32)
        y = a * acc + b
        relu = lay["relu"]
        if mutant == "no_hidden_relu" and not last:
            relu = False
        if mutant == "relu_on_plain_output" and last:
            relu = True
        if relu:
            y = torch.relu(y)
        x = y.to(dtype).to(f32)
    return x[:n].to(dtype)


@functools.lru_cache(maxsize=None)
def case_data(id, cus=ASSUMED_CUS):
    """-> (inputs, reference with bound) of the case: computed once, shared, not to be modified"""
    case = case_of(id)
    inp = make_inputs(case, cus)
    return inp, reference(inp, case["cin"], case["dtype"])
