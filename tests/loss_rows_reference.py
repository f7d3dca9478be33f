"""Float64 reference of the supervised-loss row kernels (csrc/loss_rows.hip behind include/omnipq_loss.h), the elementwise
error bounds their roundings allow, a numpy-float32 emulation of the kernels' arithmetic in their operation order, and the case
tables both suites walk (tests/test_loss_rows_reference.py on the CPU, tests/test_gpu_loss_rows_f64.py on the device).

The reference evaluates the formulas of omnipq_loss.h (and the reference's loss_helper_pq.py lines it cites) in float64 from
exactly the values the kernels read: the f32 inputs, the f32 constants float32(1e-6), float32(pi), float32(1e-8),
float32(1e-4), the f32 thresholds and class weights, and mean_size64 as float64.

Decisions.  The library is built with -ffp-contract=off and f32 division / sqrtf are correctly rounded, so everything but
expf / logf reproduces bit for bit in numpy float32: the emulation is the authority for every discrete output and decision
(label, mask, assignment, counts; the size-class argmax; the winning vote and ground-truth vote; the sign of a vote error;
the cosine's |x| > 1e-8 branch; every corner x quad gate delta < 0, w < half, pen > 1e-4; the collision count), which are
compared exactly, and the float64 reference of the continuous outputs is evaluated WITH the emulation's decisions.  The
reference also takes every decision in float64 and flags it undecided when its float64 margin is within the rounding bound of
the quantities compared; an exact tie is decided by the first-index rule when the operands are identical or the f32 values
equal the float64 ones (a lattice on which f32 arithmetic is exact).  Outside the undecided set both must agree; at most
UNDECIDED_CAP of a random case's decisions may be undecided, none of a lattice case's.

Bounds.  u = 2^-24 per f32 operation.  expf and logf are not correctly rounded: ROCm's published accuracy table gives 1 ulp
for each; every call is counted as LIBM_ULP = 2 ulp of its result, the documented figure with a factor of two over it -- a
constant of this module, never adjusted from what a device returns.  To first order, every rounding on the longest path:

    lse          a_c = s_c - mx (u |a_c| each, weighted by exp a_c / z), exp (LIBM u), n - 1 additions of positive terms:
                 rel_z = u (n - 1 + LIBM) + u sum |a_c| exp a_c / z (+ n 2^-149 / z for terms flushed to zero);
                 log (LIBM u |log z|), mx + log z (u |lse|):   e_lse = rel_z + u (LIBM |log z| + |lse|)
    CE row       lse - s[y]:   e_lse + u (|lse| + |s[y]|)  -- from |mx|, |log z| and |s[y]|, never from the difference
    term 0 row   w CE m: two more products, 2 u (|lse| + |s[y]|) w m
    smooth-L1    e carries de; the value |slope| de + u value (0.5 a is exact); a row sums 3 (2) of them: + 2 u sum
                 centre de = u |e|;  heading want = gt / (pi / nh): de = 2 u |want| + u |e|;  size de = u |gt / mean| + u |e|;
                 quad size de = u |e|
    cosine       |x|: three squares, two additions, sqrt: 2.5 u;  x_a / |x|: 3.5 u;  a product of two: 8 u;  two additions:
                 e_cs = 10 u sum_a |x_a y_a| / (|x| |y|), from the products' magnitudes;  1 - cs: + u (1 + |cs|)
    terms[h][i]  the row values are summed in f64 (no rounding to speak of): sum of the row bounds / den, + 3 u |term| for the
                 f32 cast, the f32 count + 1e-6f and the division
    CE gradient  coef: inv_mask / inv_pos 2 u, one product each with g_terms (w, m): 3 u (5 u for term 0);
                 p = exp(s - lse): argument error e_lse + u |s - lse|, exp LIBM u;  p - [c == y]: u (p + [c == y]);
                 the product: |coef| (e_p + e_sub + (crel + 1) u (p + [c == y]))
    smooth-L1 gradient   |coef| (de + 4 u |slope|): the slope is 1-Lipschitz in e, coef 3 u, the product
    cosine gradient      A = (y / |y|) / |x|: 7 u |A|;  B = cs x / |x|^2: e_cs |x_a| / |x|^2 + 8 u |B|;  A - B: u (|A| + |B|);
                 |coef| (that + 4 u (|A| + |B|)), from |A| and |B|, never from dc
    votes        g = vote_label + seed: u |g|;  |v - g|: + u |v - g|;  three of them: + 2 u dist;  loss: the rows' bounds /
                 den + 3 u loss;  gradient: 2 u |coef| (g_loss m is exact, the f32 count + 1e-6f, the division)
    physical     half = f32(size64 / 2): u;  p = +-half + centre: u |p|;  dq = -(a cx + b cy): 3 u (|a cx| + |b cy|);
                 delta = (px a + py b) + dq:  e_delta = |a| e_px + |b| e_py + 3 u (|px a| + |py b| + |a cx| + |b cy|)
      loss       a lane chains ceil(k / 256) trips x 4 corners of f32 additions, the f64 block sum, the f32 cast and one f32
                 division by n_box per quad: (sum e_delta + (4 trips + 2) u sum pen) / n_box;  the final cast: + u loss
      g_normal   terms -(p - c): e_p + u |p - c|; the lane chain 4 trips u sum |t|; cast, scale = g / n_box, product: 3 u
      g_quad_center   scale count a: 3 u |value| (the count is an integer)
      g_center, g_size   each of the four waves chains 4 ceil(q / 4) additions of -a (-a / 2), the four partials are folded
                 in f32 in a fixed order (3), scale and the product (2): (4 ceil(q / 4) + 5) u |scale| sum |a|
Structural zeros (gradients of unlabelled rows and of seeds without a vote label, non-selected class columns, z components of
the physical gradients, boxes and quads that take no part, terms[h][7], the quad call's terms[h][4..7]) must be the bits of
+0.0, not "within a bound".  All of it times MARGIN = 1.5 (decoder_reference.MARGIN) for what is not modelled.
"""
import numpy as np
import torch

from decoder_reference import MARGIN, U32, fmt, outside, ratios  # noqa: F401

F, D = np.float32, np.float64
LIBM_ULP = 2.0                      # ulp per expf / logf call: the documented 1 ulp, doubled
UNDECIDED_CAP = 0.005
TINY = 2.0 ** -149
EPS6, EPS8, PEN_THR, PI32 = F(1e-6), F(1e-8), F(1e-4), F(3.14159265358979323846)
ONE = F(1.0)
LO, HI = np.nextafter(ONE, F(0.0)), np.nextafter(ONE, F(2.0))
KINKS = np.array([0.0, LO, -LO, 1.0, -1.0, HI, -HI, 3.0, -3.0], dtype=F)
MAX_HEADS = 8
BOX_KEYS = ("objectness_scores", "center", "heading_scores", "heading_residuals_normalized", "size_scores",
            "size_residuals_normalized", "sem_cls_scores")
QUAD_KEYS = ("quad_scores", "quad_center", "normal_vector", "quad_size")
QUAD_WIDTHS = (2, 3, 3, 2)
PC_GRADS = ("g_center", "g_size_residuals", "g_quad_center", "g_normal")
NOT_SOLID = sum(1 << c for c in (5, 6, 8, 11))

MUTANTS = ("near_le", "tie_last", "numgt_le", "pos_over_mask_count", "obj_grad_no_weight", "hres_grad_col0", "heading_wrong_nh",
           "mean_of_predicted", "slope_linear", "g_terms_head0", "no_scene_offset", "cos_grad_no_norm", "vote_grad_last",
           "corner_signs_swapped", "not_solid_shifted", "quad_tile_drop_partial")


def box_widths(nh, ns, nc):
    return (2, 3, nh, nh, ns, 3 * ns, nc)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rat(got, want, bnd):
    """decoder_reference.ratios on numpy arrays"""
    return ratios({n: T(np.asarray(v, dtype=D)) for n, v in got.items()}, {n: T(np.asarray(want[n], dtype=D)) for n in got},
                  {n: T(np.asarray(bnd[n], dtype=D)) for n in got})


def plus_zero(a, where=None):
    """the selected elements of an f32 array are the bits of +0.0"""
    bits = np.ascontiguousarray(a, dtype=F).view(np.int32)
    return bool((bits == 0).all()) if where is None else bool((bits[np.broadcast_to(where, bits.shape)] == 0).all())


def exp32(x):
    """a correctly rounded expf (the kernels' is within LIBM_ULP of it)"""
    return np.exp(x.astype(D)).astype(F)


def log32(x):
    with np.errstate(divide="ignore"):
        return np.log(x.astype(D)).astype(F)


def sl1(e, mutant=None):
    """smooth-L1 with delta = 1 and its slope, in e's type"""
    a = np.abs(e)
    half = e.dtype.type(0.5)
    val = np.where(a < 1, (half * a) * a, a - half)
    slope = e if mutant == "slope_linear" else np.where(a < 1, e, np.sign(e))
    return val, slope.astype(e.dtype)


def lse32(s):
    mx = s[..., 0]
    for c in range(1, s.shape[-1]):
        mx = np.maximum(mx, s[..., c])
    z = np.zeros_like(mx)
    for c in range(s.shape[-1]):
        z = z + exp32(s[..., c] - mx)
    return mx + log32(z)


def ce_grad32(s, y, lse, coef):
    onehot = (np.arange(s.shape[-1])[None, :] == y[:, None]).astype(F)
    val = coef[:, None] * (exp32(s - lse[:, None]) - onehot)
    return np.where(coef[:, None] == 0, F(0.0), val).astype(F)


def ce_ref(s, y):
    """-> value, its bound, lse, e_lse (float64, rows)"""
    s = s.astype(D)
    n = s.shape[-1]
    mx = s.max(-1)
    a = s - mx[:, None]
    ea = np.exp(a)
    z = ea.sum(-1)
    logz = np.log(z)
    lse = mx + logz
    sy = np.take_along_axis(s, y[:, None], -1)[:, 0]
    rel_z = U32 * (n - 1 + LIBM_ULP) + U32 * (ea * np.abs(a)).sum(-1) / z + n * TINY / z
    e_lse = rel_z + U32 * (LIBM_ULP * np.abs(logz) + np.abs(lse))
    return lse - sy, e_lse + U32 * (np.abs(lse) + np.abs(sy)), lse, e_lse


def ce_grad_ref(s, y, lse, e_lse, coef, crel):
    s = s.astype(D)
    onehot = (np.arange(s.shape[-1])[None, :] == y[:, None]).astype(D)
    arg = s - lse[:, None]
    p = np.exp(arg)
    e_p = p * (e_lse[:, None] + U32 * np.abs(arg) + LIBM_ULP * U32) + TINY
    mag = p + onehot
    c = np.abs(coef)[:, None]
    return coef[:, None] * (p - onehot), c * (e_p + U32 * mag + (crel + 1) * U32 * mag)


def first_min_decided(v32, v64, e64):
    """first index of the smallest v64 along the last axis, and whether f32 arithmetic must pick the same: the minimum stands
    clear of every other candidate by more than the bounds, or every candidate in reach is exact in f32, or is an exact tie of
    identical f32 values (the first index wins in both)"""
    i64 = np.argmin(v64, -1)
    m = np.take_along_axis(v64, i64[..., None], -1)
    em = np.take_along_axis(e64, i64[..., None], -1)
    win32 = np.take_along_axis(v32, i64[..., None], -1)
    near = v64 <= m + em + e64
    exact = v32.astype(D) == v64
    same = (v64 == m) & (v32 == win32)
    decided = (near.sum(-1) == 1) | (~near | exact).all(-1) | (~near | same).all(-1)
    return i64, decided


def threshold_decided(v32, v64, e64, thr):
    """v against the f32 threshold: decided when the margin exceeds the bound or the f32 value is exact"""
    return (np.abs(v64 - D(thr)) > e64) | (v32.astype(D) == v64)


class Tally:
    """decisions taken, undecided ones, disagreements outside the undecided set"""

    def __init__(self):
        self.n = self.undecided = self.disagree = 0

    def add(self, decided, agree):
        decided, agree = np.broadcast_arrays(np.asarray(decided), np.asarray(agree))
        self.n += decided.size
        self.undecided += int((~decided).sum())
        self.disagree += int((decided & ~agree).sum())

    def share(self):
        return self.undecided / max(self.n, 1)


# ---- assignment -----------------------------------------------------------------------------------------------------------

def _sq_dist(q, g):
    dx, dy, dz = (q[:, :, None, a] - g[:, None, :, a] for a in range(3))
    d = dx * dx
    d = d + dy * dy
    return d + dz * dz


def assign_emulate(inp, mutant=None):
    q, g, num = inp["query"], inp["gt"], inp["num_gt"]
    near, far = F(inp["near"]), F(inp["far"])
    k2 = g.shape[1]
    d = _sq_dist(q, g)
    bi = (k2 - 1 - np.argmin(d[:, :, ::-1], -1)) if mutant == "tie_last" else np.argmin(d, -1)
    e = np.sqrt(np.take_along_axis(d, bi[..., None], -1)[..., 0] + EPS6)
    isnear = (e <= near) if mutant == "near_le" else (e < near)
    lab = isnear & ((bi <= num) if mutant == "numgt_le" else (bi < num))
    m = isnear | (e > far)
    return dict(label=lab.astype(np.int64), mask=m.astype(F), assignment=np.where(lab, bi, k2 - 1).astype(np.int64),
                counts=np.array([lab.sum(), m.sum()], dtype=F), bi=bi, e=e, d=d)


def assign_decisions(inp, emu):
    """the same decisions in float64 -> Tally"""
    q, g = inp["query"].astype(D), inp["gt"].astype(D)
    near, far = F(inp["near"]), F(inp["far"])
    d64 = _sq_dist(q, g)
    bi64, dec_i = first_min_decided(emu["d"], d64, 6.0 * U32 * d64)
    e64 = np.sqrt(np.take_along_axis(d64, bi64[..., None], -1)[..., 0] + D(EPS6))
    t = Tally()
    t.add(dec_i, bi64 == emu["bi"])
    for thr, got in ((near, emu["e"] < near), (far, emu["e"] > far)):
        tie = emu["e"] == thr                        # identical f32 operands: an exact tie, and both comparisons are strict
        dec = dec_i & (threshold_decided(emu["e"], e64, 4.0 * U32 * e64, thr) | tie)
        t.add(dec, np.where(tie, ~got, ((e64 < D(thr)) if thr is near else (e64 > D(thr))) == got))
    return t


def assign_inputs(c):
    rs = np.random.RandomState(c["seed"])
    b, k, k2 = c["b"], c["k"], c["k2"]
    if c["kind"] in ("lattice", "atnear"):           # multiples of 1/8: every f32 operation is exact; duplicates and equidistant slots
        g = rs.randint(-3, 4, size=(b, k2, 3)).astype(F) / F(8)
        g[:, k2 // 2] = g[:, 1]
        g[:, k2 - 1] = g[:, 0]
        q = rs.randint(-3, 4, size=(b, k, 3)).astype(F) / F(8)
        q[:, ::3] = ((g[:, 2] + g[:, 3]) / F(2))[:, None, :]          # equidistant from slots 2 and 3 (multiples of 1/16)
        q[:, 1::7] = g[:, 1][:, None, :]                              # on a duplicated slot: distance 0 twice
    else:
        g = (rs.rand(b, k2, 3) * np.array([6.0, 5.0, 2.6])).astype(F)
        if k2 >= 8:
            g[:, k2 // 2:k2 // 2 + k2 // 8] = 0.0                     # padded all-zero slots
        pick = np.arange(k) * 7 % k2
        pick[::5] = k2 - 1
        pick[1::5] = min(512, k2 - 1)
        pick[2::5] = min(1024, k2 - 1)
        spread = np.where(np.arange(k) % 3 == 0, 0.05, np.where(np.arange(k) % 3 == 1, 0.3, 1.5))[None, :, None]
        q = (g[:, pick] + spread * rs.randn(b, k, 3)).astype(F)
        q[:, -2:] = (0.05 * rs.randn(b, min(k, 2), 3)).astype(F)[:, :min(k, 2)]
    near, far = (0.6, 0.3) if c["kind"] == "nearfar" else (0.3, 0.6)
    inp = dict(query=q, gt=g, num_gt=np.zeros((b, k), dtype=np.int64), near=near, far=far, b=b, k=k, k2=k2)
    bi = assign_emulate(inp)["bi"]                   # num_gt at, just behind and far from the edge bi < num_gt
    pat = np.arange(b * k).reshape(b, k) % 4
    inp["num_gt"] = np.select([pat == 0, pat == 1, pat == 2], [np.zeros_like(bi), bi, bi + 1], k2 + 5).astype(np.int64)
    if c["kind"] == "atnear":                        # the commonest distance handed back as NEAR: e == near bit for bit, not near
        vals, cnt = np.unique(assign_emulate(inp)["e"], return_counts=True)
        cnt[vals < 0.01] = 0
        inp.update(near=float(vals[np.argmax(cnt)]), far=10.0, num_gt=np.full((b, k), k2, dtype=np.int64))
    return inp


ASSIGN_CASES = [dict(id="assign-1x1x1", b=1, k=1, k2=1, kind="random", seed=11),
                dict(id="assign-2x257x64", b=2, k=257, k2=64, kind="random", seed=12),
                dict(id="assign-3x300x513", b=3, k=300, k2=513, kind="random", seed=13),
                dict(id="assign-1x64x1100", b=1, k=64, k2=1100, kind="random", seed=14),
                dict(id="assign-lattice", b=2, k=70, k2=40, kind="lattice", seed=15),
                dict(id="assign-atnear", b=2, k=70, k2=40, kind="atnear", seed=15),
                dict(id="assign-nearfar", b=1, k=64, k2=8, kind="nearfar", seed=16)]


# ---- box rows -------------------------------------------------------------------------------------------------------------

def _gi(inp, mutant=None):
    a = np.clip(inp["assignment"], 0, inp["k2"] - 1)
    return a if mutant == "no_scene_offset" else (np.arange(inp["b"] * inp["k"]) // inp["k"]) * inp["k2"] + a


def _seq_sum(v):
    """(R, n) -> (R,): 0.f + v0 + v1 + ... in turn"""
    out = v[:, 0]
    for a in range(1, v.shape[1]):
        out = out + v[:, a]
    return out


def _finalize32(rows, counts, mutant=None):
    """rows: (8, R) f32 row values -> terms f32[8]"""
    out = np.zeros(8, dtype=F)
    for i in range(8):
        den = (counts[1] if i == 0 or mutant == "pos_over_mask_count" else counts[0]) + EPS6
        out[i] = F(rows[i].astype(D).sum()) / den
    return out


def box_emulate(inp, mutant=None):
    """-> dict(terms (H, 8) f32, grads {key: (H, R, width) f32})"""
    H, R, nh, ns, nc = inp["heads"], inp["b"] * inp["k"], inp["nh"], inp["ns"], inp["nc"]
    lab, m, counts = inp["label"] != 0, inp["mask"], inp["counts"]
    r = np.arange(R)
    inv_mask = ONE / (counts[1] + EPS6)
    inv_pos = np.where(lab, ONE / (counts[0] + EPS6), F(0.0)).astype(F)
    w = np.where(lab, inp["w"][1], inp["w"][0]).astype(F)
    y01 = lab.astype(np.int64)
    zero = F(0.0)
    terms = np.zeros((H, 8), dtype=F)
    grads = {key: np.zeros((H, R, wd), dtype=F) for key, wd in zip(BOX_KEYS, box_widths(nh, ns, nc))}
    if not inp["only_objectness"]:
        gi = _gi(inp, mutant)
        hc = np.clip(inp["gt_heading_class"][gi], 0, nh - 1)
        sc = np.clip(inp["gt_size_class"][gi], 0, ns - 1)
        ysem = np.clip(inp["gt_sem_cls"][gi], 0, nc - 1)
        want = inp["gt_heading_residual"][gi] / (PI32 / F(nh + 1 if mutant == "heading_wrong_nh" else nh))
    for h in range(H):
        gt = inp["g_terms"][0 if mutant == "g_terms_head0" else h]
        rows = np.zeros((8, R), dtype=F)
        s = inp["objectness_scores"][h]
        lse = lse32(s)
        rows[0] = w * (lse - s[r, y01]) * m
        coef = gt[0] * inv_mask * m if mutant == "obj_grad_no_weight" else gt[0] * inv_mask * w * m
        grads["objectness_scores"][h] = ce_grad32(s, y01, lse, coef.astype(F))
        if not inp["only_objectness"]:
            val, slope = sl1(inp["gt_center"][gi] - inp["center"][h], mutant)
            rows[1] = np.where(lab, _seq_sum(val), zero)
            grads["center"][h] = np.where(lab[:, None], ((-gt[1]) * inv_pos)[:, None] * slope, zero)
            for i, key, yy in ((2, "heading_scores", hc), (4, "size_scores", sc), (6, "sem_cls_scores", ysem)):
                s = inp[key][h]
                lse = lse32(s)
                rows[i] = np.where(lab, lse - s[r, yy], zero)
                grads[key][h] = ce_grad32(s, yy, lse, gt[i] * inv_pos)
            val, slope = sl1(inp["heading_residuals_normalized"][h][r, hc] - want, mutant)
            rows[3] = np.where(lab, val, zero)
            grads["heading_residuals_normalized"][h][r, 0 if mutant == "hres_grad_col0" else hc] = \
                np.where(lab, (gt[3] * inv_pos) * slope, zero)
            mrow = np.argmax(inp["size_scores"][h], -1) if mutant == "mean_of_predicted" else sc
            p = inp["size_residuals_normalized"][h].reshape(R, ns, 3)[r, sc]
            val, slope = sl1(p - inp["gt_size_residual"][gi] / inp["mean_size"][mrow], mutant)
            rows[5] = np.where(lab, _seq_sum(val), zero)
            grads["size_residuals_normalized"][h].reshape(R, ns, 3)[r, sc] = \
                np.where(lab[:, None], (gt[5] * inv_pos)[:, None] * slope, zero)
        terms[h] = _finalize32(rows, counts, mutant)
    if inp["only_objectness"]:
        grads = {"objectness_scores": grads["objectness_scores"]}
    return dict(terms=terms, grads=grads)


def _sl1_rows(e, de):
    """float64 errors e (R, n) with bounds de -> row value, row bound, slope, slope bound factor"""
    val, slope = sl1(e)
    n = e.shape[1]
    return val.sum(1), (np.abs(slope) * de + U32 * val).sum(1) + (n - 1) * U32 * val.sum(1), slope


def _finalize64(rows, erows, counts):
    terms, bnd = np.zeros(8), np.zeros(8)
    for i in range(8):
        den = D(counts[1] if i == 0 else counts[0]) + D(EPS6)
        terms[i] = rows[i].sum() / den
        bnd[i] = erows[i].sum() / den + 3.0 * U32 * abs(terms[i])
    return terms, bnd


def box_reference(inp):
    """-> (ref, bnd, zeros): terms (H, 8) and grads {key: (H, R, width)} in float64, their bounds (MARGIN included), and per
    gradient the elements the contract makes structural zeros"""
    H, R, nh, ns, nc = inp["heads"], inp["b"] * inp["k"], inp["nh"], inp["ns"], inp["nc"]
    lab, m, counts = inp["label"] != 0, inp["mask"].astype(D), inp["counts"]
    r = np.arange(R)
    inv_mask = 1.0 / (D(counts[1]) + D(EPS6))
    inv_pos = np.where(lab, 1.0 / (D(counts[0]) + D(EPS6)), 0.0)
    w = np.where(lab, inp["w"][1], inp["w"][0]).astype(D)
    y01 = lab.astype(np.int64)
    widths = box_widths(nh, ns, nc)
    terms, e_terms = np.zeros((H, 8)), np.zeros((H, 8))
    grads = {key: np.zeros((H, R, wd)) for key, wd in zip(BOX_KEYS, widths)}
    bnds = {key: np.zeros((H, R, wd)) for key, wd in zip(BOX_KEYS, widths)}
    zeros = {key: np.ones((R, wd), dtype=bool) for key, wd in zip(BOX_KEYS, widths)}
    zeros["objectness_scores"] = np.broadcast_to((m == 0)[:, None], (R, 2))
    if not inp["only_objectness"]:
        gi = _gi(inp)
        hc = np.clip(inp["gt_heading_class"][gi], 0, nh - 1)
        sc = np.clip(inp["gt_size_class"][gi], 0, ns - 1)
        ysem = np.clip(inp["gt_sem_cls"][gi], 0, nc - 1)
        want = inp["gt_heading_residual"][gi].astype(D) / (D(PI32) / nh)
        for key in ("center", "heading_scores", "size_scores", "sem_cls_scores"):
            zeros[key] = np.broadcast_to(~lab[:, None], zeros[key].shape)
        zeros["heading_residuals_normalized"] = ~lab[:, None] | (np.arange(nh)[None, :] != hc[:, None])
        zeros["size_residuals_normalized"] = ~lab[:, None] | (np.arange(3 * ns)[None, :] // 3 != sc[:, None])
    for h in range(H):
        gt = inp["g_terms"][h].astype(D)
        rows, erows = np.zeros((8, R)), np.zeros((8, R))
        s = inp["objectness_scores"][h]
        val, e_val, lse, e_lse = ce_ref(s, y01)
        sy = s.astype(D)[r, y01]
        rows[0] = w * val * m
        erows[0] = w * m * (e_val + 2.0 * U32 * (np.abs(lse) + np.abs(sy)))
        grads["objectness_scores"][h], bnds["objectness_scores"][h] = ce_grad_ref(s, y01, lse, e_lse, gt[0] * inv_mask * w * m, 5)
        if not inp["only_objectness"]:
            e = inp["gt_center"][gi].astype(D) - inp["center"][h].astype(D)
            de = U32 * np.abs(e)
            v, ev, slope = _sl1_rows(e, de)
            rows[1], erows[1] = lab * v, lab * ev
            coef = (-gt[1] * inv_pos)[:, None]
            grads["center"][h], bnds["center"][h] = coef * slope, np.abs(coef) * (de + 4.0 * U32 * np.abs(slope))
            for i, key, yy in ((2, "heading_scores", hc), (4, "size_scores", sc), (6, "sem_cls_scores", ysem)):
                val, e_val, lse, e_lse = ce_ref(inp[key][h], yy)
                rows[i], erows[i] = lab * val, lab * e_val
                grads[key][h], bnds[key][h] = ce_grad_ref(inp[key][h], yy, lse, e_lse, gt[i] * inv_pos, 3)
            e = (inp["heading_residuals_normalized"][h].astype(D)[r, hc] - want)[:, None]
            de = 2.0 * U32 * np.abs(want)[:, None] + U32 * np.abs(e)
            v, ev, slope = _sl1_rows(e, de)
            rows[3], erows[3] = lab * v, lab * ev
            coef = gt[3] * inv_pos
            grads["heading_residuals_normalized"][h][r, hc] = coef * slope[:, 0]
            bnds["heading_residuals_normalized"][h][r, hc] = np.abs(coef) * (de[:, 0] + 4.0 * U32 * np.abs(slope[:, 0]))
            q = inp["gt_size_residual"][gi].astype(D) / inp["mean_size"].astype(D)[sc]
            e = inp["size_residuals_normalized"][h].astype(D).reshape(R, ns, 3)[r, sc] - q
            de = U32 * (np.abs(q) + np.abs(e))
            v, ev, slope = _sl1_rows(e, de)
            rows[5], erows[5] = lab * v, lab * ev
            coef = (gt[5] * inv_pos)[:, None]
            grads["size_residuals_normalized"][h].reshape(R, ns, 3)[r, sc] = coef * slope
            bnds["size_residuals_normalized"][h].reshape(R, ns, 3)[r, sc] = np.abs(coef) * (de + 4.0 * U32 * np.abs(slope))
        terms[h], e_terms[h] = _finalize64(rows, erows, counts)
    if inp["only_objectness"]:
        grads, bnds, zeros = ({"objectness_scores": x["objectness_scores"]} for x in (grads, bnds, zeros))
    return (dict(terms=terms, grads=grads), dict(terms=MARGIN * e_terms, grads={k: MARGIN * v for k, v in bnds.items()}), zeros)


def _scores(rs, kind, shape):
    """randn | pm60: every logit +-60 (a dominated row whenever the signs differ) | equal | onelow: one column far below"""
    s = rs.randn(*shape)
    if kind == "pm60":
        s = np.where(rs.rand(*shape) < 0.5, 60.0, -60.0)
    elif kind == "equal":
        s = np.full(shape, 0.75)
    elif kind == "onelow":
        s[..., rs.randint(0, shape[-1])] = -40.0
    else:
        assert kind == "randn", kind
    return s.astype(F)


def _labels(rs, R, labels, mask):
    lab = dict(mixed=rs.rand(R) < 0.5, none=np.zeros(R, bool), all=np.ones(R, bool))[labels]
    if labels == "mixed":
        lab[0] = True
    m = dict(mixed=lab | (rs.rand(R) < 0.3), zero=np.zeros(R, bool))[mask]
    return lab.astype(np.int64), m.astype(F), np.array([lab.sum(), m.sum()], dtype=F)


def _g_terms(rs, H):
    """zeros, negatives, another row of 8 per head"""
    g = (rs.randn(H, 8) + 0.5 * np.arange(H)[:, None]).astype(F)
    g[::2, 3] = 0.0
    g[1::3, 4] = 0.0
    g[:, 1] = -np.abs(g[:, 1])
    return g


def _kinks(R, n, shift):
    return KINKS[(np.arange(R)[:, None] * n + np.arange(n)[None, :] + shift) % len(KINKS)]


def _nulls(keys, H, pattern, rot):
    """the (key, head) pairs whose gradient pointer is NULL"""
    if pattern == "all":
        return set()
    if pattern == "none":
        return {(key, h) for key in keys for h in range(H)}
    assert pattern == "rot", pattern
    return {(key, h) for i, key in enumerate(keys) for h in range(H) if (i + h + rot) % 3 == 0}


def box_inputs(c):
    rs = np.random.RandomState(c["seed"])
    b, k, k2, H = c["b"], c["k"], c["k2"], c["heads"]
    nh, ns, nc = c["dims"]
    R = b * k
    only = bool(c.get("only_objectness"))
    lab, m, counts = _labels(rs, R, c.get("labels", "mixed"), c.get("mask", "mixed"))
    inp = dict(b=b, k=k, k2=k2, heads=H, nh=nh, ns=ns, nc=nc, only_objectness=int(only), label=lab, mask=m, counts=counts,
               assignment=rs.randint(0, k2, size=R).astype(np.int64), w=np.array([0.2, 0.8], dtype=F), g_terms=_g_terms(rs, H),
               nulls=_nulls(BOX_KEYS[:1] if only else BOX_KEYS, H, c.get("ptrs", "all"), c["seed"]))
    kind = c.get("scores", "randn")
    inp["objectness_scores"] = _scores(rs, kind, (H, R, 2))
    if only:
        return inp
    G = b * k2
    mean = (0.3 + 1.7 * rs.rand(ns, 3)).astype(F)
    inp.update(gt_center=rs.randn(G, 3).astype(F), gt_heading_class=(np.arange(G) * 5 % nh).astype(np.int64),
               gt_heading_residual=((2.0 * rs.rand(G) - 1.0) * np.pi / nh).astype(F),
               gt_size_class=(np.arange(G) * 7 % ns).astype(np.int64), gt_sem_cls=(np.arange(G) * 3 % nc).astype(np.int64),
               mean_size=mean)
    inp["gt_size_residual"] = (0.2 * rs.randn(G, 3) * mean[inp["gt_size_class"]]).astype(F)
    if c.get("clamp"):                              # out of range both ways: the clamped label is what counts
        inp["assignment"][::3] = k2 + 2
        inp["assignment"][1::3] = -1
        for key, n in (("gt_heading_class", nh), ("gt_size_class", ns), ("gt_sem_cls", nc)):
            inp[key][::2] = n + 3
            inp[key][1::4] = -2
    gi = _gi(inp)
    sc = np.clip(inp["gt_size_class"][gi], 0, ns - 1)
    hc = np.clip(inp["gt_heading_class"][gi], 0, nh - 1)
    inp["center"] = (inp["gt_center"][gi][None] + 0.8 * rs.randn(H, R, 3)).astype(F)
    inp["heading_scores"] = _scores(rs, kind, (H, R, nh))
    inp["heading_residuals_normalized"] = (0.8 * rs.randn(H, R, nh)).astype(F)
    inp["size_scores"] = _scores(rs, kind, (H, R, ns))
    inp["size_residuals_normalized"] = (0.8 * rs.randn(H, R, 3 * ns)).astype(F)
    inp["sem_cls_scores"] = _scores(rs, kind, (H, R, nc))
    if c.get("resid") == "kink":                    # ground-truth residuals 0: e is the stored prediction, exactly
        inp["gt_center"][:] = 0.0
        inp["gt_heading_residual"][:] = 0.0
        inp["gt_size_residual"][:] = 0.0
        r = np.arange(R)
        for h in range(H):
            inp["center"][h] = _kinks(R, 3, h)
            inp["heading_residuals_normalized"][h][r, hc] = _kinks(R, 1, h + 4)[:, 0]
            inp["size_residuals_normalized"][h].reshape(R, ns, 3)[r, sc] = _kinks(R, 3, h + 2)
    return inp


def _box(id, b, k, k2, heads, dims, seed, **kw):
    return dict(id=id, b=b, k=k, k2=k2, heads=heads, dims=dims, seed=seed, **kw)


BOX_CASES = [
    _box("box-R1-h1-w1", 1, 1, 1, 1, (1, 1, 1), 21, labels="all"),
    _box("box-R255-h3-randn", 3, 85, 64, 3, (12, 18, 18), 22, ptrs="rot"),
    _box("box-R256-h8-pm60", 2, 128, 64, 8, (64, 64, 64), 23, scores="pm60"),
    _box("box-R257-h1-equal", 257, 1, 1, 1, (5, 64, 2), 24, scores="equal", ptrs="rot"),
    _box("box-R513-h3-kink", 3, 171, 64, 3, (12, 18, 18), 25, scores="onelow", resid="kink", ptrs="rot"),
    _box("box-R80-h8-kink-w1", 2, 40, 64, 8, (1, 1, 1), 26, resid="kink"),
    _box("box-nopos", 2, 40, 8, 3, (12, 18, 18), 27, labels="none"),
    _box("box-allpos", 2, 40, 8, 3, (12, 18, 18), 28, labels="all"),
    _box("box-maskzero", 2, 40, 8, 3, (12, 18, 18), 29, mask="zero"),
    _box("box-clamp", 2, 40, 8, 3, (12, 18, 18), 30, clamp=True),
    _box("box-nullall", 2, 40, 8, 3, (5, 64, 2), 31, ptrs="none"),
    _box("box-onlyobj-h7", 2, 128, 1, 7, (1, 1, 1), 32, only_objectness=True),
    _box("box-onlyobj-null", 3, 85, 1, 8, (1, 1, 1), 33, only_objectness=True, ptrs="none", scores="pm60"),
]


def box_clamped_twin(inp):
    """the same problem with every label already clamped: must give the same result, bit for bit"""
    twin = dict(inp)
    twin["assignment"] = np.clip(inp["assignment"], 0, inp["k2"] - 1)
    for key, n in (("gt_heading_class", inp["nh"]), ("gt_size_class", inp["ns"]), ("gt_sem_cls", inp["nc"])):
        twin[key] = np.clip(inp[key], 0, n - 1)
    return twin


# ---- quad rows ------------------------------------------------------------------------------------------------------------

NORMAL_KINDS = ("randn", "zero", "tiny", "parallel", "antiparallel", "zero_gt")


def _norm3(x):
    return np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])


def quad_emulate(inp, mutant=None):
    H, R = inp["heads"], inp["b"] * inp["k"]
    lab, m, counts = inp["label"] != 0, inp["mask"], inp["counts"]
    r = np.arange(R)
    gi = _gi(inp, mutant)
    inv_mask = ONE / (counts[1] + EPS6)
    inv_pos = np.where(lab, ONE / (counts[0] + EPS6), F(0.0)).astype(F)
    w = np.where(lab, inp["w"][1], inp["w"][0]).astype(F)
    y01 = lab.astype(np.int64)
    zero = F(0.0)
    terms = np.zeros((H, 8), dtype=F)
    grads = {key: np.zeros((H, R, wd), dtype=F) for key, wd in zip(QUAD_KEYS, QUAD_WIDTHS)}
    branch = np.zeros((H, R), dtype=bool)
    for h in range(H):
        gt = inp["g_terms"][0 if mutant == "g_terms_head0" else h]
        rows = np.zeros((8, R), dtype=F)
        s = inp["quad_scores"][h]
        lse = lse32(s)
        rows[0] = w * (lse - s[r, y01]) * m
        coef = gt[0] * inv_mask * m if mutant == "obj_grad_no_weight" else gt[0] * inv_mask * w * m
        grads["quad_scores"][h] = ce_grad32(s, y01, lse, coef.astype(F))
        val, slope = sl1(inp["gt_center"][gi] - inp["quad_center"][h], mutant)
        rows[1] = np.where(lab, _seq_sum(val), zero)
        grads["quad_center"][h] = np.where(lab[:, None], ((-gt[1]) * inv_pos)[:, None] * slope, zero)
        x, y = inp["normal_vector"][h], inp["gt_normal"][gi]
        nx, ny = _norm3(x), _norm3(y)
        dx, dy = np.maximum(nx, EPS8), np.maximum(ny, EPS8)
        xs, ys = x / dx[:, None], y / dy[:, None]
        cs = xs[:, 0] * ys[:, 0] + xs[:, 1] * ys[:, 1] + xs[:, 2] * ys[:, 2]
        rows[2] = np.where(lab, ONE - cs, zero)
        branch[h] = nx > EPS8
        dc = ys / dx[:, None]
        if mutant != "cos_grad_no_norm":
            with np.errstate(divide="ignore", invalid="ignore"):
                dc = np.where(branch[h][:, None], dc - cs[:, None] * x / (nx * nx)[:, None], dc)
        grads["normal_vector"][h] = np.where(lab[:, None], ((-gt[2]) * inv_pos)[:, None] * dc, zero)
        val, slope = sl1(inp["quad_size"][h] - inp["gt_size"][gi], mutant)
        rows[3] = np.where(lab, _seq_sum(val), zero)
        grads["quad_size"][h] = np.where(lab[:, None], (gt[3] * inv_pos)[:, None] * slope, zero)
        terms[h] = _finalize32(rows, counts, mutant)
    return dict(terms=terms, grads=grads, branch=branch)


def quad_reference(inp, branch):
    """branch (H, R): the emulation's |x| > 1e-8 decisions -> (ref, bnd, zeros, tally)"""
    H, R = inp["heads"], inp["b"] * inp["k"]
    lab, m, counts = inp["label"] != 0, inp["mask"].astype(D), inp["counts"]
    r = np.arange(R)
    gi = _gi(inp)
    inv_mask = 1.0 / (D(counts[1]) + D(EPS6))
    inv_pos = np.where(lab, 1.0 / (D(counts[0]) + D(EPS6)), 0.0)
    w = np.where(lab, inp["w"][1], inp["w"][0]).astype(D)
    y01 = lab.astype(np.int64)
    terms, e_terms = np.zeros((H, 8)), np.zeros((H, 8))
    grads = {key: np.zeros((H, R, wd)) for key, wd in zip(QUAD_KEYS, QUAD_WIDTHS)}
    bnds = {key: np.zeros((H, R, wd)) for key, wd in zip(QUAD_KEYS, QUAD_WIDTHS)}
    zeros = {key: np.broadcast_to(~lab[:, None], (R, wd)) for key, wd in zip(QUAD_KEYS, QUAD_WIDTHS)}
    zeros["quad_scores"] = np.broadcast_to((m == 0)[:, None], (R, 2))
    tally = Tally()
    for h in range(H):
        gt = inp["g_terms"][h].astype(D)
        rows, erows = np.zeros((8, R)), np.zeros((8, R))
        s = inp["quad_scores"][h]
        val, e_val, lse, e_lse = ce_ref(s, y01)
        sy = s.astype(D)[r, y01]
        rows[0] = w * val * m
        erows[0] = w * m * (e_val + 2.0 * U32 * (np.abs(lse) + np.abs(sy)))
        grads["quad_scores"][h], bnds["quad_scores"][h] = ce_grad_ref(s, y01, lse, e_lse, gt[0] * inv_mask * w * m, 5)
        for i, key, e, sign in ((1, "quad_center", inp["gt_center"][gi].astype(D) - inp["quad_center"][h].astype(D), -1.0),
                                (3, "quad_size", inp["quad_size"][h].astype(D) - inp["gt_size"][gi].astype(D), 1.0)):
            de = U32 * np.abs(e)
            v, ev, slope = _sl1_rows(e, de)
            rows[i], erows[i] = lab * v, lab * ev
            coef = (sign * gt[i] * inv_pos)[:, None]
            grads[key][h], bnds[key][h] = coef * slope, np.abs(coef) * (de + 4.0 * U32 * np.abs(slope))
        x, y = inp["normal_vector"][h].astype(D), inp["gt_normal"][gi].astype(D)
        nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
        tally.add(threshold_decided(_norm3(inp["normal_vector"][h]), nx, 2.5 * U32 * nx, EPS8), (nx > D(EPS8)) == branch[h])
        dx, dy = np.where(branch[h], nx, D(EPS8)), np.maximum(ny, D(EPS8))
        prod = x * y / (dx * dy)[:, None]
        cs, e_cs = prod.sum(1), 10.0 * U32 * np.abs(prod).sum(1)
        rows[2], erows[2] = lab * (1.0 - cs), lab * (e_cs + U32 * (1.0 + np.abs(cs)))
        A = y / (dy * dx)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            B = np.where(branch[h][:, None], cs[:, None] * x / (nx * nx)[:, None], 0.0)
            eB = np.where(branch[h][:, None], e_cs[:, None] * np.abs(x) / (nx * nx)[:, None], 0.0) + 8.0 * U32 * np.abs(B)
        mag = np.abs(A) + np.abs(B)
        coef = (-gt[2] * inv_pos)[:, None]
        grads["normal_vector"][h] = coef * (A - B)
        bnds["normal_vector"][h] = np.abs(coef) * (7.0 * U32 * np.abs(A) + eB + U32 * mag + 4.0 * U32 * mag)
        terms[h], e_terms[h] = _finalize64(rows, erows, counts)
    return (dict(terms=terms, grads=grads), dict(terms=MARGIN * e_terms, grads={k: MARGIN * v for k, v in bnds.items()}), zeros,
            tally)


def quad_inputs(c):
    rs = np.random.RandomState(c["seed"])
    b, k, k2, H = c["b"], c["k"], c["k2"], c["heads"]
    R, G = b * k, b * k2
    lab, m, counts = _labels(rs, R, c.get("labels", "all"), c.get("mask", "mixed"))
    inp = dict(b=b, k=k, k2=k2, heads=H, label=lab, mask=m, counts=counts, w=np.array([0.4, 0.6], dtype=F), g_terms=_g_terms(rs, H),
               nulls=_nulls(QUAD_KEYS, H, c.get("ptrs", "all"), c["seed"]), assignment=rs.randint(0, k2, size=R).astype(np.int64),
               gt_center=rs.randn(G, 3).astype(F), gt_size=(1.0 + rs.rand(G, 2)).astype(F))
    gn = rs.randn(G, 3)
    inp["gt_normal"] = (gn / np.linalg.norm(gn, axis=1, keepdims=True)).astype(F)
    kinds = np.arange(R) % len(NORMAL_KINDS)
    inp["gt_normal"].reshape(b, k2, 3)[:, k2 - 1] = 0.0          # an assigned padded slot
    inp["assignment"][kinds == 5] = k2 - 1
    if c.get("clamp"):
        inp["assignment"][kinds == 0] = k2 + 7
        inp["assignment"][kinds == 3] = -4
    gi = _gi(inp)
    inp["quad_scores"] = _scores(rs, c.get("scores", "randn"), (H, R, 2))
    inp["quad_center"] = (inp["gt_center"][gi][None] + 0.8 * rs.randn(H, R, 3)).astype(F)
    inp["quad_size"] = (inp["gt_size"][gi][None] + 0.8 * rs.randn(H, R, 2)).astype(F)
    nv = rs.randn(H, R, 3).astype(F)
    y = inp["gt_normal"][gi]
    scale = (0.5 + rs.rand(H, R, 1)).astype(F)
    nv[:, kinds == 1] = 0.0
    nv[:, kinds == 2] *= F(1e-9) / np.linalg.norm(nv[:, kinds == 2], axis=-1, keepdims=True).astype(F)
    nv[:, kinds == 3] = (scale * y[None])[:, kinds == 3]
    nv[:, kinds == 4] = (-scale * y[None])[:, kinds == 4]
    inp["normal_vector"] = nv.astype(F)
    if c.get("resid") == "kink":
        inp["gt_center"][:] = 0.0
        inp["gt_size"][:] = 0.0
        for h in range(H):
            inp["quad_center"][h] = _kinks(R, 3, h)
            inp["quad_size"][h] = _kinks(R, 2, h + 5)
    return inp


def _quad(id, b, k, k2, heads, seed, **kw):
    return dict(id=id, b=b, k=k, k2=k2, heads=heads, seed=seed, **kw)


QUAD_CASES = [
    _quad("quad-R1-h1", 1, 1, 1, 1, 41),
    _quad("quad-R256-h7", 2, 128, 32, 7, 42, ptrs="rot"),
    _quad("quad-R257-h8-kink", 257, 1, 4, 8, 43, resid="kink", scores="pm60"),
    _quad("quad-R513-h1-mixed", 3, 171, 32, 1, 44, labels="mixed", clamp=True, scores="onelow"),
    _quad("quad-nopos", 2, 40, 8, 7, 45, labels="none", ptrs="rot"),
    _quad("quad-nullall", 2, 40, 8, 8, 46, ptrs="none", scores="equal"),
]


# ---- votes ----------------------------------------------------------------------------------------------------------------

def _vote_geometry(inp, dtype):
    b, s, n, vf, gv = inp["dims"]
    Tn = b * s
    src = np.clip(inp["seed_inds"].astype(np.int64), 0, n - 1)
    row = (np.arange(Tn) // max(s, 1)) * n + src
    m = inp["vote_label_mask"][row] != 0
    g = inp["vote_label"][row].reshape(Tn, gv, 3).astype(dtype) + inp["seed_xyz"].astype(dtype)[:, None, :]
    v = inp["vote_xyz"].reshape(Tn, vf, 3).astype(dtype)
    a = np.abs(v[:, :, None, :] - g[:, None, :, :])                     # (T, vf, gv, 3)
    return m, g, v, (a[..., 0] + a[..., 1]) + a[..., 2], a


def votes_emulate(inp, mutant=None):
    b, s, n, vf, gv = inp["dims"]
    Tn = b * s
    t = np.arange(Tn)
    m, g, v, dd, _ = _vote_geometry(inp, F)
    ddj = np.swapaxes(dd, 1, 2)                                        # (T, gv, vf)
    ij = (vf - 1 - np.argmin(ddj[:, :, ::-1], -1)) if mutant == "vote_grad_last" else np.argmin(ddj, -1)
    dj = np.take_along_axis(ddj, ij[..., None], -1)[..., 0]
    bj = np.argmin(dj, -1)
    bi, dist = ij[t, bj], dj[t, bj]
    mf = m.astype(F)
    sums = np.array([(dist * mf).astype(D).sum(), mf.astype(D).sum()])
    loss = F(sums[0]) / (F(sums[1]) + EPS6)
    coef = (inp["g_loss"] * mf) / (F(sums[1]) + EPS6)
    sign = np.sign(v - g[t, bj][:, None, :]).astype(F)
    hit = (np.arange(vf)[None, :] == bi[:, None]) & m[:, None]
    grad = np.where(hit[..., None], coef[:, None, None] * sign, F(0.0)).astype(F)
    return dict(loss=np.array([loss], dtype=F), grad=grad.reshape(Tn * vf, 3), bi=bi, bj=bj, sign=sign[t, bi], dd=dd, m=m)


def votes_reference(inp, emu):
    b, s, n, vf, gv = inp["dims"]
    Tn = b * s
    t = np.arange(Tn)
    m, g, v, dd, a = _vote_geometry(inp, D)
    e_dd = U32 * (np.abs(g)[:, None, :, :] + a).sum(-1) + 2.0 * U32 * dd
    bi, bj = emu["bi"], emu["bj"]
    dist, e_dist = dd[t, bi, bj], e_dd[t, bi, bj]
    cnt = m.astype(D).sum()
    den = D(F(cnt)) + D(EPS6)
    loss = (dist * m).sum() / den
    e_loss = (e_dist * m).sum() / den + 3.0 * U32 * abs(loss)
    coef = D(inp["g_loss"]) * m / den
    hit = (np.arange(vf)[None, :] == bi[:, None]) & m[:, None]
    grad = np.where(hit[..., None], (coef[:, None] * emu["sign"].astype(D))[:, None, :], 0.0)
    bnd = np.where(hit[..., None], 2.0 * U32 * np.abs(coef)[:, None, None], 0.0) * np.ones(3)
    # the same decisions in float64
    tally = Tally()
    ddj, e_ddj, dd32 = np.swapaxes(dd, 1, 2), np.swapaxes(e_dd, 1, 2), np.swapaxes(emu["dd"], 1, 2)
    ij64, dec_i = first_min_decided(dd32, ddj, e_ddj)
    pick = lambda x: np.take_along_axis(x, ij64[..., None], -1)[..., 0]                      # noqa: E731
    bj64, dec_j = first_min_decided(pick(dd32), pick(ddj), pick(e_ddj))
    dec = dec_i.all(-1) & dec_j
    tally.add(dec, (bj64 == bj) & (ij64[t, bj64] == bi))
    ex64 = (v - g[t, bj][:, None, :])[t, bi]
    ex32 = (inp["vote_xyz"].reshape(Tn, vf, 3) - (inp["vote_label"][_vote_row(inp)].reshape(Tn, gv, 3)
                                                  + inp["seed_xyz"][:, None, :])[t, bj][:, None, :])[t, bi]
    dec_s = (np.abs(ex64) > U32 * np.abs(g[t, bj])) | (ex32.astype(D) == ex64)
    tally.add(dec_s, np.sign(ex64) == emu["sign"])
    return (dict(loss=np.array([loss]), grad=grad.reshape(Tn * vf, 3)),
            dict(loss=MARGIN * np.array([e_loss]), grad=MARGIN * bnd.reshape(Tn * vf, 3)), ~hit.repeat(3).reshape(Tn * vf, 3), tally)


def _vote_row(inp):
    b, s, n, vf, gv = inp["dims"]
    return (np.arange(b * s) // max(s, 1)) * n + np.clip(inp["seed_inds"].astype(np.int64), 0, n - 1)


def votes_inputs(c):
    rs = np.random.RandomState(c["seed"])
    b, s, n, vf, gv = c["dims"]
    Tn = b * s
    kind = c.get("kind", "random")
    inp = dict(dims=c["dims"], seed_xyz=(rs.rand(Tn, 3) * np.array([6.0, 5.0, 2.6])).astype(F),
               seed_inds=rs.randint(0, n, size=Tn).astype(np.int32), vote_label=(0.4 * rs.randn(b * n, 3 * gv)).astype(F),
               vote_label_mask=(rs.rand(b * n) < 0.6).astype(np.int64) * 3, g_loss=F(c.get("g_loss", 0.7)))
    if kind == "equal":                             # multiples of 2^-10: the target vote_label + seed_xyz is exact in f32
        for key in ("seed_xyz", "vote_label"):
            inp[key] = (np.round(inp[key] * 1024.0) / 1024.0).astype(F)
    if kind == "clamp":
        inp["seed_inds"][::2] = -1
        inp["seed_inds"][1::4] = n
        inp["vote_label_mask"].reshape(b, n)[:, [0, n - 1]] = 1
    if kind == "mask0":
        inp["vote_label_mask"][:] = 0
    if kind == "dupgt":
        inp["vote_label"][:, 3:6] = inp["vote_label"][:, 0:3]
    inp["vote_xyz"] = (np.repeat(inp["seed_xyz"], vf, axis=0) + 0.3 * rs.randn(Tn * vf, 3)).astype(F)
    if kind == "dupvotes":
        inp["vote_xyz"].reshape(Tn, vf, 3)[:, 1:] = inp["vote_xyz"].reshape(Tn, vf, 3)[:, :1]
    if kind == "equal":                             # a vote on its target (rows 0 mod 3), one coordinate on it (rows 1 mod 3)
        g = inp["vote_label"][_vote_row(inp)].reshape(Tn, gv, 3) + inp["seed_xyz"][:, None, :]
        v = inp["vote_xyz"].reshape(Tn, vf, 3)
        v[::3, 0] = g[::3, gv - 1]
        v[1::3, :, 0] = g[1::3, :1, 0]
    return inp


def _votes(id, dims, seed, **kw):
    return dict(id=id, dims=dims, seed=seed, **kw)


VOTE_CASES = [
    _votes("votes-1x1x1-f1-g1", (1, 1, 1, 1, 1), 51),
    _votes("votes-2x257x300-f1-g3", (2, 257, 300, 1, 3), 52),
    _votes("votes-2x100x150-f3-g3", (2, 100, 150, 3, 3), 53, g_loss=-1.3),
    _votes("votes-1x65x70-f2-g8", (1, 65, 70, 2, 8), 54),
    _votes("votes-1x33x40-f1-g1", (1, 33, 40, 1, 1), 55),
    _votes("votes-clamp", (2, 33, 40, 2, 3), 56, kind="clamp"),
    _votes("votes-mask0", (2, 33, 40, 2, 3), 57, kind="mask0", g_loss=-1.3),
    _votes("votes-dupvotes", (2, 33, 40, 3, 3), 58, kind="dupvotes"),
    _votes("votes-dupgt", (2, 33, 40, 2, 3), 59, kind="dupgt"),
    _votes("votes-equal", (2, 33, 40, 2, 3), 60, kind="equal"),
]


# ---- physical constraints -------------------------------------------------------------------------------------------------

PC_THREADS, PC_BOXES, PC_TILE = 256, 64, 256


def _pc_boxes(inp, mutant=None):
    """the pre-pass: class, footprint and use of every box (the size in float64, as the reference keeps the class means)"""
    b, k, k2, ns, q = inp["dims"]
    cls = np.argmax(inp["size_scores"], -1)                                        # first maximum; exact comparisons
    res = np.take_along_axis(inp["size_residuals"], cls[..., None, None], 2)[:, :, 0]
    size64 = inp["mean_size64"][cls][..., :2] + res[..., :2].astype(D)
    sem = np.take_along_axis(inp["sem_cls_label"], np.clip(inp["object_assignment"], 0, k2 - 1), 1)
    inside = (sem >= 0) & (sem < 64)
    sh = np.where(inside, sem, 0).astype(np.uint64) + np.uint64(1 if mutant == "not_solid_shifted" else 0)
    bit = (np.uint64(inp["not_solid"]) >> np.minimum(sh, np.uint64(63))) & np.uint64(1)
    bit = np.where(sh > 63, np.uint64(0), bit)
    use = (inp["object_label"] != 0) & ~(inside & (bit != 0))
    return cls, size64 / 2.0, use


def _pc_pairs(inp, half64, dtype):
    """every (scene, quad, box, corner): px, py, delta, w in `dtype`, the kernels' operation order"""
    hl, hw = (half64[..., i].astype(F).astype(dtype) if dtype is F else half64[..., i] for i in (0, 1))
    bx, by = inp["center"][..., 0].astype(dtype), inp["center"][..., 1].astype(dtype)
    sx, sy = np.array([1, 1, -1, -1], dtype=dtype), np.array([1, -1, 1, -1], dtype=dtype)
    px = (sx * hl[..., None] + bx[..., None])[:, None]                              # (b, 1, k, 4)
    py = (sy * hw[..., None] + by[..., None])[:, None]
    a, bq = (inp["normal_vector"][..., i].astype(dtype)[:, :, None, None] for i in (0, 1))
    cx, cy = (inp["quad_center"][..., i].astype(dtype)[:, :, None, None] for i in (0, 1))
    dq = -(a * cx + bq * cy)
    delta = (px * a + py * bq) + dq
    kk = -delta
    ex, ey = (px + a * kk) - cx, (py + bq * kk) - cy
    return dict(px=px, py=py, a=a, bq=bq, cx=cx, cy=cy, dq=dq, delta=delta, kk=kk, ex=ex, ey=ey, w=np.sqrt(ex * ex + ey * ey),
                half=inp["quad_size"][..., 0].astype(dtype)[:, :, None, None], hl=hl, hw=hw)


def _lane_chain(terms, k):
    """(b, q, k, 4) f32 -> (b, q): lane l adds its boxes l, l + 256, ... corner by corner in f32, the block sums in f64"""
    b, q = terms.shape[:2]
    acc = np.zeros((b, q, PC_THREADS), dtype=F)
    for i0 in range(0, k, PC_THREADS):
        n = min(PC_THREADS, k - i0)
        for c in range(4):
            acc[:, :, :n] = acc[:, :, :n] + terms[:, :, i0:i0 + n, c]
    return acc.astype(D).sum(-1)


def pc_emulate(inp, mutant=None):
    b, k, k2, ns, q = inp["dims"]
    cls, half64, use = _pc_boxes(inp, mutant)
    n_box = use.sum(1).astype(F)
    g = _pc_pairs(inp, half64, F)
    neg, inside = g["delta"] < 0, g["w"] < g["half"]
    live = (inp["quad_label"] != 0)[:, :, None, None] & (n_box != 0)[:, None, None, None] & use[:, None, :, None]
    gate = neg & inside & live
    pen = np.where(gate, g["kk"], F(0.0)).astype(F)
    hits = gate & (pen > PEN_THR)
    zero = F(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = n_box[:, None]
        tot = _lane_chain(pen, k)
        per_quad = np.where(tot != 0, (tot.astype(F) / inv).astype(D), 0.0)
        out = np.array([per_quad.sum(), hits.sum()], dtype=D).astype(F)
        # backward, quad side
        qlive = (inp["quad_label"] != 0) & (n_box != 0)[:, None]
        scale = np.where(qlive, inp["g_out"] / inv, zero).astype(F)
        sa = _lane_chain(np.where(gate, -(g["px"] - g["cx"]), zero).astype(F), k).astype(F)
        sb = _lane_chain(np.where(gate, -(g["py"] - g["cy"]), zero).astype(F), k).astype(F)
        sc = gate.sum((2, 3)).astype(F)
        a0 = np.where(qlive, inp["normal_vector"][..., 0], zero)
        b0 = np.where(qlive, inp["normal_vector"][..., 1], zero)
        g_normal = np.stack([scale * sa, scale * sb, np.zeros_like(sa)], -1).astype(F)
        g_qc = np.stack([scale * sc * a0, scale * sc * b0, np.zeros_like(sa)], -1).astype(F)
        # backward, box side: wave = quad % 4 (the tile of 256 is a multiple of 4), corners in turn, the partials folded in order
        part = np.zeros((4, 4, b, k), dtype=F)                                        # [wave][gx, gy, gl, gw]
        q_eff = q // PC_TILE * PC_TILE if mutant == "quad_tile_drop_partial" else q
        sx, sy = (1, 1, -1, -1), (1, -1, 1, -1)
        gsx, gsy = (sy, sx) if mutant == "corner_signs_swapped" else (sx, sy)
        for t in range(q_eff):
            p = part[t % 4]
            a, bq = g["a"][:, t, 0, 0][:, None], g["bq"][:, t, 0, 0][:, None]
            for c in range(4):
                h = gate[:, t, :, c]
                p[0] = np.where(h, p[0] - a, p[0])
                p[1] = np.where(h, p[1] - bq, p[1])
                p[2] = np.where(h, p[2] - F(0.5) * F(gsx[c]) * a, p[2])
                p[3] = np.where(h, p[3] - F(0.5) * F(gsy[c]) * bq, p[3])
        tot4 = ((part[0] + part[1]) + part[2]) + part[3]
        bscale = np.where(use & (n_box != 0)[:, None], inp["g_out"] / inv, zero).astype(F)
    g_center = np.stack([bscale * tot4[0], bscale * tot4[1], np.zeros_like(bscale)], -1).astype(F)
    g_size = np.zeros((b, k, ns, 3), dtype=F)
    bi, ki = np.meshgrid(np.arange(b), np.arange(k), indexing="ij")
    g_size[bi, ki, cls, 0] = bscale * tot4[2]
    g_size[bi, ki, cls, 1] = bscale * tot4[3]
    return dict(out=out, g_center=g_center, g_size_residuals=g_size, g_quad_center=g_qc, g_normal=g_normal, cls=cls, use=use,
                gate=gate, hits=hits, neg=neg, inside=inside, geo=g, live=live)


def pc_reference(inp, emu):
    """float64 with the emulation's class, use and gates -> (ref, bnd, zeros, tally)"""
    b, k, k2, ns, q = inp["dims"]
    cls, use, gate = emu["cls"], emu["use"], emu["gate"]
    _, half64, _ = _pc_boxes(inp)
    n_box = use.sum(1).astype(D)
    g = _pc_pairs(inp, half64, D)
    ab = np.abs
    e_px = U32 * ab(g["hl"])[:, None, :, None] + U32 * ab(g["px"])
    e_py = U32 * ab(g["hw"])[:, None, :, None] + U32 * ab(g["py"])
    mags = ab(g["px"] * g["a"]) + ab(g["py"] * g["bq"]) + ab(g["a"] * g["cx"]) + ab(g["bq"] * g["cy"])
    e_delta = ab(g["a"]) * e_px + ab(g["bq"]) * e_py + 3.0 * U32 * mags
    trips = (k + PC_THREADS - 1) // PC_THREADS
    pen = np.where(gate, g["kk"], 0.0)
    qlive = (inp["quad_label"] != 0) & (n_box != 0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(n_box != 0, 1.0 / n_box, 0.0)[:, None]
        per_quad = pen.sum((2, 3)) * inv
        e_quad = ((e_delta * gate).sum((2, 3)) + (4 * trips + 2) * U32 * pen.sum((2, 3))) * inv
        loss = per_quad.sum()
        ref = dict(out=np.array([loss, emu["hits"].sum()], dtype=D))
        bnd = dict(out=np.array([e_quad.sum() + U32 * abs(loss), 0.0]))
        scale = np.where(qlive, D(inp["g_out"]) * inv, 0.0)
        gn, en = np.zeros((b, q, 3)), np.zeros((b, q, 3))
        for i, (p, c, ep) in enumerate(((g["px"], g["cx"], e_px), (g["py"], g["cy"], e_py))):
            t = np.where(gate, -(p - c), 0.0)
            gn[..., i] = scale * t.sum((2, 3))
            en[..., i] = ab(scale) * (((ep + U32 * ab(p - c)) * gate).sum((2, 3)) + (4 * trips + 3) * U32 * ab(t).sum((2, 3)))
        cnt = gate.sum((2, 3)).astype(D)
        gq = np.stack([scale * cnt * g["a"][:, :, 0, 0], scale * cnt * g["bq"][:, :, 0, 0], np.zeros((b, q))], -1)
        bscale = np.where(use & (n_box != 0)[:, None], D(inp["g_out"]) * inv, 0.0)
        depth = 4 * ((q + 3) // 4) + 5
        gc, ec = np.zeros((b, k, 3)), np.zeros((b, k, 3))
        gs, es = np.zeros((b, k, ns, 3)), np.zeros((b, k, ns, 3))
        bi, ki = np.meshgrid(np.arange(b), np.arange(k), indexing="ij")
        sx, sy = np.array([1.0, 1.0, -1.0, -1.0]), np.array([1.0, -1.0, 1.0, -1.0])
        for i, (n, sg) in enumerate(((g["a"], sx), (g["bq"], sy))):
            nn = np.broadcast_to(n, gate.shape)
            gc[..., i] = bscale * np.where(gate, -nn, 0.0).sum((1, 3))
            ec[..., i] = ab(bscale) * depth * U32 * np.where(gate, ab(nn), 0.0).sum((1, 3))
            gs[bi, ki, cls, i] = bscale * np.where(gate, -0.5 * sg * nn, 0.0).sum((1, 3))
            es[bi, ki, cls, i] = 0.5 * ec[..., i]
    ref.update(g_center=gc, g_size_residuals=gs, g_quad_center=gq, g_normal=gn)
    bnd.update(g_center=ec, g_size_residuals=es, g_quad_center=3.0 * U32 * ab(gq), g_normal=en)
    zc = np.zeros((b, k, 3), dtype=bool)
    zc[..., 2] = True
    zc |= ~(use & (n_box != 0)[:, None])[..., None]
    zs = np.ones((b, k, ns, 3), dtype=bool)
    zs[bi, ki, cls, 0] = zc[..., 0]
    zs[bi, ki, cls, 1] = zc[..., 0]
    zq = np.zeros((b, q, 3), dtype=bool)
    zq[..., 2] = True
    zq |= ~qlive[..., None]
    zeros = dict(g_center=zc, g_size_residuals=zs, g_quad_center=zq, g_normal=zq)
    # the gates in float64, on the pairs that take part
    live, g32 = np.broadcast_to(emu["live"], gate.shape), emu["geo"]
    tally = Tally()
    dec_d = threshold_decided(g32["delta"], g["delta"], e_delta, F(0.0))
    e_ex = e_px + ab(g["a"]) * e_delta + U32 * (ab(g["a"] * g["kk"]) + ab(g["ex"] + g["cx"]) + ab(g["ex"]))
    e_ey = e_py + ab(g["bq"]) * e_delta + U32 * (ab(g["bq"] * g["kk"]) + ab(g["ey"] + g["cy"]) + ab(g["ey"]))
    dec_w = dec_d & threshold_decided(g32["w"], g["w"], e_ex + e_ey + 2.5 * U32 * g["w"], 0.0) \
        & ((ab(g["w"] - g["half"]) > e_ex + e_ey + 2.5 * U32 * g["w"]) | (g32["w"].astype(D) == g["w"]))
    dec_p = dec_d & threshold_decided(g32["kk"], g["kk"], e_delta, PEN_THR)
    neg64, in64 = g["delta"] < 0, g["w"] < g["half"]
    tally.add(dec_d[live], (neg64 == emu["neg"])[live])
    sel = live & neg64 & emu["neg"]
    tally.add(dec_w[sel], (in64 == emu["inside"])[sel])
    sel = sel & in64 & emu["inside"]
    tally.add(dec_p[sel], ((g["kk"] > D(PEN_THR)) == emu["hits"])[sel])
    return ref, {n: MARGIN * v for n, v in bnd.items()}, zeros, tally


def pc_inputs(c):
    rs = np.random.RandomState(c["seed"])
    b, k, k2, ns, q = c["dims"]
    kind = c.get("kind", "random")
    if kind == "lattice":
        return _pc_lattice(c)
    room = np.array([6.0, 5.0, 2.6])
    center = rs.rand(b, k, 3) * room
    hug = rs.rand(b, k) < 0.5                                         # half of the boxes hug a wall and poke through it
    wall = rs.randint(0, 4, size=(b, k))
    off = 0.3 * rs.rand(b, k)
    center[..., 0] = np.where(hug & (wall == 0), off, np.where(hug & (wall == 1), room[0] - off, center[..., 0]))
    center[..., 1] = np.where(hug & (wall == 2), off, np.where(hug & (wall == 3), room[1] - off, center[..., 1]))
    qc, qn, qs = np.zeros((b, q, 3)), np.zeros((b, q, 3)), np.zeros((b, q, 2))
    walls = [([0, 2.5, 1.3], [1, 0, 0], 5.0), ([6, 2.5, 1.3], [-1, 0, 0], 5.0), ([3, 0, 1.3], [0, 1, 0], 6.0), ([3, 5, 1.3], [0, -1, 0], 6.0)]
    for j in range(q):
        if j % 3 == 0:
            cc, nn, ss = walls[(j // 3) % 4]
            qc[:, j], qn[:, j], qs[:, j] = cc, nn, (ss, 2.6)
        else:                                                         # oblique partitions
            ang = rs.rand(b) * 2 * np.pi
            qc[:, j] = np.stack([1 + 4 * rs.rand(b), 1 + 3 * rs.rand(b), np.full(b, 1.3)], -1)
            qn[:, j] = np.stack([np.cos(ang), np.sin(ang), np.zeros(b)], -1)
            qs[:, j] = np.stack([1 + rs.rand(b), np.full(b, 2.6)], -1)
    qn += 0.05 * rs.randn(b, q, 3)
    inp = dict(dims=c["dims"], center=center.astype(F), size_scores=rs.randn(b, k, ns).astype(F),
               size_residuals=(0.2 * rs.randn(b, k, ns, 3)).astype(F), object_label=(rs.rand(b, k) < 0.6).astype(np.int64) * 2,
               object_assignment=rs.randint(0, k2, size=(b, k)).astype(np.int64),
               sem_cls_label=rs.randint(0, 18, size=(b, k2)).astype(np.int64), mean_size64=0.3 + 1.7 * rs.rand(ns, 3),
               quad_center=qc.astype(F), normal_vector=qn.astype(F), quad_size=qs.astype(F),
               quad_label=(rs.rand(b, q) < 0.7).astype(np.int64), not_solid=NOT_SOLID, g_out=F(c.get("g_out", 0.7)))
    inp["object_label"][:, 0] = 1
    inp["quad_label"][:, 0] = 1
    if kind == "nosolid":                           # scene 0 has no box that takes part, scene 1 has some
        inp["object_label"][0] = 0
    if kind == "noquads":
        inp["quad_label"][:] = 0
    if kind == "bit63":
        inp["not_solid"] = NOT_SOLID | (1 << 63)
        inp["sem_cls_label"][:, ::3] = 63
    if kind == "outside":                           # class ids outside 0..63: solid
        inp["sem_cls_label"][:, ::3] = 64
        inp["sem_cls_label"][:, 1::3] = -1
        inp["not_solid"] = (1 << 64) - 1
        inp["sem_cls_label"][:, 2::3] = 7
        inp["object_assignment"][:, ::2] = k2 + 3
        inp["object_assignment"][:, 1::4] = -2
    if kind == "ties":
        inp["size_scores"][:, ::2] = F(0.5)
        top = inp["size_scores"][:, 1::2].max(-1) + F(1.0)
        inp["size_scores"][:, 1::2, 1] = top
        inp["size_scores"][:, 1::2, ns - 1] = top
    return inp


def _pc_lattice(c):
    """an axis-aligned room: walls on integers, half sizes and centres on multiples of 1/8, every product exact.  Corners ON a
    wall (penetration exactly 0: no hit), projections exactly AT half (not inside) and one f32 step inside, and two boxes whose
    corner is 1677 and 1678 steps of 2^-24 behind the wall x = 0: just below and just above float32(1e-4)"""
    b, k, k2, ns, q = c["dims"]
    rs = np.random.RandomState(c["seed"])
    assert b == 1 and ns == 3 and q == 8
    mean64 = np.array([[1.0, 0.5, 1.0], [0.5, 0.25, 1.0], [2.0, 1.0, 1.0]])
    center = np.zeros((1, k, 3))
    center[0, :, 0] = rs.randint(-4, 37, size=k) / 8.0
    center[0, :, 1] = rs.randint(-4, 29, size=k) / 8.0
    scores = np.zeros((1, k, 3), dtype=F)
    scores[0, np.arange(k), np.arange(k) % 3] = 1.0
    res = np.zeros((1, k, 3, 3), dtype=F)
    res[0, ::2, :, :2] = 0.25
    step = 2.0 ** -24
    for i, n in ((0, 1677), (1, 1678)):             # class 0, no residual: half length 0.5; corner x = -n 2^-24
        scores[0, i] = (1.0, 0.0, 0.0)
        res[0, i] = 0.0
        center[0, i, :2] = (-0.5 - n * step, 1.5)
    qc = np.array([[0, 1.5, 1.3], [4, 1.5, 1.3], [2, 0, 1.3], [2, 3, 1.3]] * 2, dtype=D)[None]
    qn = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]] * 2, dtype=D)[None]
    qs = np.array([[2.0, 2.6]] * 4 + [[np.nextafter(F(2.0), F(3.0)), 2.6]] * 4, dtype=F)[None]
    return dict(dims=c["dims"], center=center.astype(F), size_scores=scores, size_residuals=res,
                object_label=np.ones((1, k), dtype=np.int64), object_assignment=np.zeros((1, k), dtype=np.int64),
                sem_cls_label=np.zeros((1, k2), dtype=np.int64), mean_size64=mean64, quad_center=qc.astype(F),
                normal_vector=qn.astype(F), quad_size=qs, quad_label=np.ones((1, 8), dtype=np.int64), not_solid=NOT_SOLID,
                g_out=F(0.7))


def _pc(id, dims, seed, **kw):
    return dict(id=id, dims=dims, seed=seed, **kw)


PC_CASES = [
    _pc("pc-1x1x1-s1-q1", (1, 1, 1, 1, 1), 71),
    _pc("pc-2x63-q5", (2, 63, 8, 3, 5), 72),
    _pc("pc-2x64-q5", (2, 64, 8, 3, 5), 73, g_out=-1.3),
    _pc("pc-2x65-q5", (2, 65, 8, 3, 5), 74),
    _pc("pc-2x513-q7", (2, 513, 64, 18, 7), 75),
    _pc("pc-2x40-q257", (2, 40, 64, 18, 257), 76),
    _pc("pc-1x20-q600", (1, 20, 8, 3, 600), 77),
    _pc("pc-nosolid", (2, 65, 8, 3, 5), 78, kind="nosolid"),
    _pc("pc-noquads", (2, 65, 8, 3, 5), 79, kind="noquads"),
    _pc("pc-bit63", (2, 65, 64, 3, 5), 80, kind="bit63"),
    _pc("pc-outside", (2, 65, 64, 3, 5), 81, kind="outside"),
    _pc("pc-ties", (2, 65, 8, 18, 5), 82, kind="ties"),
    _pc("pc-lattice", (1, 48, 1, 3, 8), 83, kind="lattice"),
]
LATTICE_CASES = ("assign-lattice", "assign-atnear", "pc-lattice")
ALL_CASES = ASSIGN_CASES + BOX_CASES + QUAD_CASES + VOTE_CASES + PC_CASES


def case_of(id):
    return next(c for c in ALL_CASES if c["id"] == id)


def ids(cases):
    return [c["id"] for c in cases]
