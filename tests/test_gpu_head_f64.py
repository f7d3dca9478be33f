"""GPU: the prediction-head and vote decode kernels (csrc/head_ops.hip) through the C ABI against the float64 reference,
ELEMENT BY ELEMENT.

Every entry point of head_ops.hip is called directly, in both libraries (bfloat16 and IEEE half), on buffers laid out as in
test_gpu_decoder_f64: each buffer, input or output, sits between two guard bands and is filled with a NaN pattern
beforehand; every output has one spare row that must keep the pattern.  Every element a kernel owns must be finite and inside
the bound tests/head_reference.py derives from the kernel's roundings (no exceptions, no norms), every guard must still hold
the pattern, pass-through outputs and zero padding are compared bit for bit, the spare columns of the input rows are NaN (a
kernel that reads them poisons its result), and the gradients arrive through descriptors of every kind (dense e16 / f32,
absent, an expanded scalar, a non-contiguous view).  The cases are head_reference's tables; the CPU suite holds an emulation
of the kernels' arithmetic, and thirteen mutants of it, against the same bounds on the same cases
(tests/test_head_reference.py).  The single backward entry points never accumulate, so a case whose dbase accumulates runs
through omnipq_decode_pair_bwd with the smallest problem of the other head beside it.

Each test prints the largest error / bound ratio per output (`RATIO <library> <case>: center=... hr=...`, pytest -s).
Largest ratios per library and output over all cases, measured on an MI355X (bfloat16 | half, the case that set it):
    object head   center  0.666 | 0.666   head-w79-3x85-tie-rot0        hr     0.616 | 0.648   head-w97-3x85-zeros-rot4, w138-3x1
                  sr      0.666 | 0.664   head-w97-3x85-zeros-rot4      pred   0.620 | 0.620   head-w12-3x85-last-rot1, w79-3x85
                  dy      0.663 | 0.661   head-w97-2x5-last-rot3        dbase  0.646 | 0.646   head-w79-2x5-random-rot4 (0: copies)
    quad head     norm    0.609 | 0.578   quad-R1023-offset, R257       normal 0.594 | 0.562   quad-R1023-offset, R257-offset
                  center  0.667 | 0.667   quad-R1025-randn              dy     0.661 | 0.662   quad-R1281-randn, R1281-dominated
                  dbase   0.667 | 0.667   quad-R2304-dominated
    pair          the same outputs at or below the single kernels' ratios (q_norm 0.389 | 0.344, q_normal 0.492 | 0.416)
    group of 5    dy 0.659 | 0.650   q_dy 0.639 | 0.649   sink 0.119 | 0.119   own dbase / q_dbase 0 (copies)
    vote          vote_xyz 0.666 | 0.666  vote-2x77-C8, C1              norm   0.156 | 0.183   vote-2x31-C8
                  out     0.662 | 0.661   vote-3x33-C288, 2x31-C288     twin   0.664 | 0.662   vote-3x33-C320, 1x32-C67
                  dnet    0.664 | 0.663   vote-2x77-C67, 3x33-C288      dseed  0.663 | 0.663   vote-3x33-C288
    vote rows     vote_xyz 0.662 | 0.663  rows-131-C288                 norm   0.101 | 0.130   rows-131-C288, rows-131-C8
                  out     0.663 | 0.660   rows-131-C288, C320           dnet, dseed  0.663 | 0.661   rows-131-C288
Nothing is above 1 / MARGIN and no guard was touched: the suite found no defect in head_ops.hip.  An e16 store or a single f32
operation at its worst rounding sits at 1 / MARGIN of its bound; the sums (norm, sink) stay far below bounds that count every
rounding of the longest path at its worst.  The emulation's table (tests/test_head_reference.py) is the same to three digits.
"""
import ctypes

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import head_reference as hr
from test_gpu_decoder_f64 import Buf, P, IN, LIBS, LIB_IDS, lib_of, same_bits

pytestmark = pytest.mark.gpu
F32 = torch.float32
IDS = lambda cases: [c["id"] for c in cases]                                   # noqa: E731


def libname(dtype):
    return LIB_IDS[LIBS.index(dtype)]


def report(dtype, id, rat):
    print(f"\n  RATIO {libname(dtype)} {id}: {hr.fmt(rat)}")
    assert not hr.outside(rat), (libname(dtype), id, hr.outside(rat))
    assert max(r[0] for r in rat.values()) <= 1.0 / hr.MARGIN, (libname(dtype), id, hr.fmt(rat))


def OUT(rows, width, dtype):
    """an output of `rows` rows and one spare row"""
    return Buf((rows + 1) * width, dtype)


def read(buf, rows, width):
    assert buf.pattern_from(rows * width), "wrote behind the last row"
    return buf.get(rows, width, numel=rows * width)


def ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[0 if b is None else b.ptr().value for b in bufs])


def ints(values):
    return (ctypes.c_int * len(values))(*values)


def intact(buf, src):
    return buf.guards_intact() and same_bits(buf.get(buf.n), src.reshape(-1))


def grad_args(grads):
    """-> (the buffers, strides [n][4], n2 [n], e16 flags [n]) of a list of head_reference.Grad"""
    bufs = [IN(g.storage) for g in grads]
    strides = [s for g in grads for s in (g.sb, g.sk, g.s1, g.s2)]
    return bufs, strides, [g.n2 for g in grads], [int(g.storage is not None and g.storage.dtype is not F32) for g in grads]


def grads_intact(bufs, grads):
    return all(b is None or intact(b, g.storage) for b, g in zip(bufs, grads))


def zero_bits(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


# ---- the two heads: buffers, calls, checks ----------------------------------------------------------------------------------

def head_fwd_bufs(inp, dtype):
    R = inp["B"] * inp["K"]
    return dict(y=IN(inp["y"]), base=IN(inp["base"]), means=IN(inp["means"]),
                outs=[OUT(R, wd, F32 if name in hr.HEAD_F32 else dtype)
                      for name, wd in zip(hr.HEAD_OUTPUTS, hr.head_out_widths(*inp["dims"]))])


def check_head_fwd(inp, b, dtype):
    R = inp["B"] * inp["K"]
    got = {name: read(buf, R, wd) for name, buf, wd in zip(hr.HEAD_OUTPUTS, b["outs"], hr.head_out_widths(*inp["dims"]))}
    assert intact(b["y"], inp["y"]) and intact(b["base"], inp["base"]) and intact(b["means"], inp["means"])
    ref = hr.head_reference(inp)
    for name in hr.HEAD_BITS:
        assert same_bits(got[name], ref[name]), name
    return hr.ratios({n: got[n] for n in hr.HEAD_BOUNDED}, ref, hr.head_bounds(ref, dtype)), got


def quad_fwd_bufs(inp, dtype):
    R = inp["B"] * inp["K"]
    return dict(y=IN(inp["y"]), base=IN(inp["base"]), norm=Buf(2, F32),
                outs=[OUT(R, wd, F32 if name == "center" else dtype) for name, wd in zip(hr.QUAD_OUTPUTS, hr.QUAD_WIDTHS)])


def check_quad_fwd(inp, b, dtype):
    R = inp["B"] * inp["K"]
    got = {name: read(buf, R, wd) for name, buf, wd in zip(hr.QUAD_OUTPUTS, b["outs"], hr.QUAD_WIDTHS)}
    got["norm"] = read(b["norm"], 1, 1).reshape(1)
    assert intact(b["y"], inp["y"]) and intact(b["base"], inp["base"])
    ref = hr.quad_reference(inp)
    assert same_bits(got["scores"], ref["scores"]) and same_bits(got["size"], ref["size"])
    assert hr.norm_round_trips(got["norm"], dtype), "the stored norm is no e16 number"
    return hr.ratios({n: got[n] for n in ("norm", "center", "normal")}, ref, hr.quad_bounds(ref, dtype)), got


def bwd_problem(inp, grads, lddy, dbase, prior, norm_in=None):
    return dict(inp=inp, grads=grads, lddy=lddy, dbase=dbase, prior=prior if dbase == "acc" else None, norm_in=norm_in)


def bwd_bufs(p, dtype, own_dbase=True):
    R = p["inp"]["B"] * p["inp"]["K"]
    g, strides, n2, flags = grad_args(p["grads"])
    b = dict(y=IN(p["inp"]["y"]), g=g, strides=strides, n2=n2, flags=flags, dy=OUT(R, p["lddy"], dtype),
             dbase=Buf(3 * R + 3, F32, p["prior"]) if own_dbase and p["dbase"] != "null" else None)
    if "means" in p["inp"]:
        b["means"] = IN(p["inp"]["means"])
    else:
        b["norm"] = IN(torch.tensor([p["norm_in"]], dtype=F32))
    return b


def check_bwd(p, b, dtype):
    """either head's backward: dy and dbase against the reference, the padding +0 bit for bit, the inputs untouched"""
    inp, head = p["inp"], "means" in p["inp"]
    R = inp["B"] * inp["K"]
    w = hr.head_width(*inp["dims"]) if head else 10
    got = dict(dy=read(b["dy"], R, p["lddy"]))
    assert zero_bits(got["dy"][:, w:]), "padding columns are not +0"
    if head:
        ref = hr.head_bwd_reference(inp, p["grads"], p["lddy"], p["prior"])
        assert intact(b["means"], inp["means"])
    else:
        ref = hr.quad_bwd_reference(inp, p["grads"], p["lddy"], p["norm_in"], p["prior"])
        assert intact(b["norm"], torch.tensor([p["norm_in"]], dtype=F32))
    if b["dbase"] is not None:
        got["dbase"] = read(b["dbase"], R, 3)
    assert intact(b["y"], inp["y"]) and grads_intact(b["g"], p["grads"])
    return hr.ratios(got, ref, hr.head_bwd_bounds(ref, dtype))


def head_bwd_tail(b, p):
    return (ptrs(b["g"]), ints(b["strides"]), ints(b["n2"]), ints(b["flags"]), P(b["dy"]), p["lddy"], P(b["dbase"]))


def quad_bwd_tail(b, p):
    return (ptrs(b["g"]), ints(b["strides"]), ints(b["flags"]), P(b["dy"]), p["lddy"], P(b["dbase"]))


def call_pair_bwd(lib, stream, hp, hb, qp, qb):
    hi, qi = hp["inp"], qp["inp"]
    acc = int(hp["dbase"] == "acc") | int(qp["dbase"] == "acc") << 1
    rc = lib.omnipq_decode_pair_bwd(hi["B"] * hi["K"], hi["K"], *hi["dims"], P(hb["y"]), hi["ldy"], P(hb["means"]), hi["hr_scale"],
                                    *head_bwd_tail(hb, hp), qi["B"] * qi["K"], qi["K"], P(qb["y"]), qi["ldy"], P(qb["norm"]),
                                    *quad_bwd_tail(qb, qp), acc, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()


def small_quad_problem(dtype):
    c = hr.case_of("quad-R1-randn")
    inp, grads = hr.quad_case_inputs(c, dtype)
    return bwd_problem(inp, grads, c["lddy"], "fresh", None, hr.quad_case_norm(c, inp, dtype))


def small_head_problem(dtype):
    c = hr.case_of("head-w12-1x1-zeros-rot2")
    inp, grads = hr.head_case_inputs(c, dtype)
    return bwd_problem(inp, grads, c["lddy"], "fresh", None)


# ---- object head ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", IDS(hr.HEAD_CASES))
def test_object_head_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    case = hr.case_of(id)
    inp, grads = hr.head_case_inputs(case, dtype)
    R = case["B"] * case["K"]
    b = head_fwd_bufs(inp, dtype)
    rc = lib.omnipq_head_decode(R, *case["dims"], P(b["y"]), case["ldy"], P(b["base"]), P(b["means"]), inp["hr_scale"],
                                ptrs(b["outs"]), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    rat, _ = check_head_fwd(inp, b, dtype)
    hp = bwd_problem(inp, grads, case["lddy"], case["dbase"], hr.dbase_prior(case, R))
    hb = bwd_bufs(hp, dtype)
    if case["dbase"] == "acc":
        qp = small_quad_problem(dtype)
        qb = bwd_bufs(qp, dtype)
        call_pair_bwd(lib, stream, hp, hb, qp, qb)
        assert not hr.outside(check_bwd(qp, qb, dtype))
    else:
        rc = lib.omnipq_head_decode_bwd(R, case["K"], *case["dims"], P(hb["y"]), case["ldy"], P(hb["means"]), inp["hr_scale"],
                                        *head_bwd_tail(hb, hp), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
    rat.update(check_bwd(hp, hb, dtype))
    assert set(rat) == set(hr.HEAD_BOUNDED) | {"dy"} | (set() if case["dbase"] == "null" else {"dbase"})
    report(dtype, id, rat)


# ---- quad head ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", IDS(hr.QUAD_CASES))
def test_quad_head_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    case = hr.case_of(id)
    inp, grads = hr.quad_case_inputs(case, dtype)
    R = case["R"]
    b = quad_fwd_bufs(inp, dtype)
    rc = lib.omnipq_quad_decode(R, P(b["y"]), case["ldy"], P(b["base"]), ptrs(b["outs"]), P(b["norm"]), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    rat, _ = check_quad_fwd(inp, b, dtype)
    qp = bwd_problem(inp, grads, case["lddy"], case["dbase"], hr.dbase_prior(case, R), hr.quad_case_norm(case, inp, dtype))
    qb = bwd_bufs(qp, dtype)
    if case["dbase"] == "acc":
        hp = small_head_problem(dtype)
        hb = bwd_bufs(hp, dtype)
        call_pair_bwd(lib, stream, hp, hb, qp, qb)
        assert not hr.outside(check_bwd(hp, hb, dtype))
    else:
        rc = lib.omnipq_quad_decode_bwd(R, case["K"], P(qb["y"]), case["ldy"], P(qb["norm"]), *quad_bwd_tail(qb, qp), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
    rat.update(check_bwd(qp, qb, dtype))
    assert set(rat) == {"norm", "center", "normal", "dy"} | (set() if case["dbase"] == "null" else {"dbase"})
    report(dtype, id, rat)


# ---- both heads in one launch ---------------------------------------------------------------------------------------------

def pair_problems(case, dtype):
    B, Kh, Kq, dims = (case[n] for n in ("B", "Kh", "Kq", "dims"))
    w = hr.head_width(*dims)
    hi = hr.head_inputs(dims, B, Kh, (w + 7) // 8 * 8, case["score"], dtype, case["seed"])
    qi = hr.quad_inputs(B, Kq, 32, "dominated" if B * Kq > 1024 else "randn", dtype, case["seed"] + 1)
    return hi, qi


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("pos16", [False, True], ids=["pos", "pos16"])
@pytest.mark.parametrize("id", IDS(hr.PAIR_CASES))
def test_decode_pair_every_element_is_inside_its_bound(id, pos16, dtype):
    lib, stream = lib_of(dtype)
    case = next(c for c in hr.PAIR_CASES if c["id"] == id)
    B, Kh, Kq = case["B"], case["Kh"], case["Kq"]
    hi, qi = pair_problems(case, dtype)
    hb, qb = head_fwd_bufs(hi, dtype), quad_fwd_bufs(qi, dtype)
    rows, kpad = B * (Kh + Kq), 32
    pos, p16 = OUT(rows, 3, F32), OUT(rows, kpad, dtype) if pos16 else None
    head = (B * Kh, Kh, *case["dims"], P(hb["y"]), hi["ldy"], P(hb["base"]), P(hb["means"]), hi["hr_scale"], ptrs(hb["outs"]),
            B * Kq, Kq, P(qb["y"]), qi["ldy"], P(qb["base"]), ptrs(qb["outs"]), P(qb["norm"]), P(pos))
    rc = lib.omnipq_decode_pair_pos16(*head, P(p16), kpad, stream) if pos16 else lib.omnipq_decode_pair(*head, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    rat, hgot = check_head_fwd(hi, hb, dtype)
    qrat, qgot = check_quad_fwd(qi, qb, dtype)
    rat.update({"q_" + n: r for n, r in qrat.items()})
    got = read(pos, rows, 3).reshape(B, Kh + Kq, 3)                               # the centres again, side by side per scene
    assert same_bits(got[:, :Kh].contiguous(), hgot["center"].reshape(B, Kh, 3))
    assert same_bits(got[:, Kh:].contiguous(), qgot["center"].reshape(B, Kq, 3))
    if pos16:
        g16 = read(p16, rows, kpad)
        assert same_bits(g16[:, :3].contiguous(), got.reshape(rows, 3).to(dtype)) and zero_bits(g16[:, 3:])
    report(dtype, f"{id}-{'pos16' if pos16 else 'pos'}", rat)


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("i", range(len(hr.PAIR_CASES)), ids=IDS(hr.PAIR_CASES))
def test_decode_pair_bwd_every_element_is_inside_its_bound(i, dtype):
    lib, stream = lib_of(dtype)
    case = hr.PAIR_CASES[i]
    B, Kh, Kq, dims = (case[n] for n in ("B", "Kh", "Kq", "dims"))
    hi, qi = pair_problems(case, dtype)
    prior = hr.dbase_prior(dict(dbase="acc", seed=case["seed"]), B * max(Kh, Kq))
    hp = bwd_problem(hi, hr.head_grads(dims, B, Kh, case["rot"], dtype, case["seed"] + 2), hr.head_width(*dims) + 3,
                     ("acc", "fresh")[i], prior[:B * Kh])
    qp = bwd_problem(qi, hr.quad_grads(B, Kq, case["rot"] + 1, dtype, case["seed"] + 3), 16, ("fresh", "acc")[i], prior[:B * Kq],
                     hr.quad_case_norm(dict(norm="own"), qi, dtype))
    hb, qb = bwd_bufs(hp, dtype), bwd_bufs(qp, dtype)
    call_pair_bwd(lib, stream, hp, hb, qp, qb)
    rat = check_bwd(hp, hb, dtype)
    rat.update({"q_" + n: r for n, r in check_bwd(qp, qb, dtype).items()})
    assert set(rat) == {"dy", "dbase", "q_dy", "q_dbase"}
    report(dtype, case["id"] + "-bwd", rat)


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("sink", [True, False], ids=["sink", "own"])
def test_decode_pair_group_bwd_every_element_is_inside_its_bound(sink, dtype):
    lib, stream = lib_of(dtype)
    case = hr.GROUP_CASE
    n, B, Kh, Kq, dims = (case[m] for m in ("n", "B", "Kh", "Kq", "dims"))
    w, Rh = hr.head_width(*dims), B * Kh
    hps, qps = [], []
    for s in range(n):
        seed = case["seed"] + 10 * s
        hi = hr.head_inputs(dims, B, Kh, w + 7, hr.SCORE_KINDS[s], dtype, seed)
        qi = hr.quad_inputs(B, Kq, 10, hr.QUAD_KINDS[s % 3], dtype, seed + 1)
        hps.append(bwd_problem(hi, hr.head_grads(dims, B, Kh, s, dtype, seed + 2), w + 3, "fresh", None))
        qps.append(bwd_problem(qi, hr.quad_grads(B, Kq, s + 2, dtype, seed + 3), 35, "null" if s == 1 else "fresh", None,
                               hr.quad_case_norm(dict(norm="any"), qi, dtype)))
    hbs = [bwd_bufs(p, dtype, own_dbase=not sink) for p in hps]
    qbs = [bwd_bufs(p, dtype) for p in qps]
    prior = hr.dbase_prior(dict(dbase="acc", seed=case["seed"]), Rh)
    sink_buf = Buf(3 * Rh + 3, F32, prior) if sink else None
    hi, qi = hps[0]["inp"], qps[0]["inp"]
    rc = lib.omnipq_decode_pair_group_bwd(
        n, Rh, Kh, *dims, ptrs([b["y"] for b in hbs]), hi["ldy"], ptrs([b["means"] for b in hbs]), hi["hr_scale"],
        ptrs([g for b in hbs for g in b["g"]]), ints([s for b in hbs for s in b["strides"]]), ints(hbs[0]["n2"]),
        ints([f for b in hbs for f in b["flags"]]), ptrs([b["dy"] for b in hbs]), hps[0]["lddy"],
        ctypes.c_void_p(0) if sink else ptrs([b["dbase"] for b in hbs]), B * Kq, Kq, ptrs([b["y"] for b in qbs]), qi["ldy"],
        ptrs([b["norm"] for b in qbs]), ptrs([g for b in qbs for g in b["g"]]), ints([s for b in qbs for s in b["strides"]]),
        ints([f for b in qbs for f in b["flags"]]), ptrs([b["dy"] for b in qbs]), qps[0]["lddy"], ptrs([b["dbase"] for b in qbs]),
        P(sink_buf), int(sink), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    worst = {}
    for s in range(n):
        rat = check_bwd(hps[s], hbs[s], dtype)
        rat.update({"q_" + m: r for m, r in check_bwd(qps[s], qbs[s], dtype).items()})
        assert set(rat) == {"dy", "q_dy"} | (set() if sink else {"dbase"}) | (set() if s == 1 else {"q_dbase"}), s
        assert not hr.outside(rat), (s, rat)
        for m, r in rat.items():
            worst[m] = r if m not in worst or r[0] > worst[m][0] else worst[m]
    if sink:
        centre = [hr.grad_values(p["grads"][1], B, Kh, 3) for p in hps]
        want, bnd = hr.sink_reference(centre, prior)
        worst.update(hr.ratios(dict(sink=read(sink_buf, Rh, 3)), dict(sink=want), dict(sink=bnd)))
    report(dtype, f"{case['id']}-{'sink' if sink else 'own'}", worst)


# ---- vote decode, channel-major -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", IDS(hr.VOTE_CASES))
def test_vote_decode_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    case = hr.case_of(id)
    B, K, C = case["B"], case["K"], case["C"]
    N = B * K
    inp, bi, ft = hr.vote_case_inputs(case, dtype)
    e16 = ft is not F32
    if case["layout"].startswith("cm"):
        feat, strides = hr.to_channel_major(inp["seed"], B, K), (C * K, K, 1)
    else:
        feat, strides = inp["seed"], (K * C, 1, C)
    net, sx, sf = IN(inp["net"]), IN(inp["seed_xyz"]), IN(feat)
    vx, out, twin, norm = OUT(N, 3, F32), OUT(N, C, ft), OUT(N, C, dtype), OUT(N, 1, F32)
    rc = lib.omnipq_vote_decode(B, K, C, P(net), case["ld"], P(sx), P(sf), int(e16), *strides, P(vx), P(out), P(twin), P(norm),
                                stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(vote_xyz=read(vx, N, 3), norm=read(norm, N, 1).reshape(N), twin=read(twin, N, C),
               out=hr.to_point_major(read(out, N, C).reshape(B, C, K)))
    assert intact(net, inp["net"]) and intact(sx, inp["seed_xyz"]) and intact(sf, feat)
    assert same_bits(got["twin"], got["out"].to(dtype)), "twin is not the e16 rounding of the kernel's own out"
    depth = hr.vote_depth(C, rows=False)
    ref = hr.vote_reference(inp)
    rat = hr.ratios(got, ref | dict(twin=ref["out"]), hr.vote_bounds(ref, dtype, depth, e16))
    ob, nb = IN(hr.to_channel_major(bi["out"], B, K)), IN(bi["norm"])
    gx = IN(bi["g_xyz"])
    g = None if bi["g"] is None else IN(hr.to_channel_major(bi["g"], B, K))
    dnet, dseed = OUT(N, case["ldd"], dtype), OUT(N, C, ft) if bi["dseed"] else None
    rc = lib.omnipq_vote_decode_bwd(B, K, C, P(ob), int(e16), P(nb), P(gx), P(g), P(dnet), case["ldd"], P(dseed), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    bgot = dict(dnet=read(dnet, N, case["ldd"]))
    assert zero_bits(bgot["dnet"][:, 3 + C:]), "padding columns are not +0"
    if dseed is not None:
        bgot["dseed"] = hr.to_point_major(read(dseed, N, C).reshape(B, C, K))
    assert ob.guards_intact() and nb.guards_intact() and (gx is None or gx.guards_intact()) and (g is None or g.guards_intact())
    bref = hr.vote_bwd_reference(bi)
    bref["dseed"] = bref["dv"]
    rat.update(hr.ratios(bgot, bref, hr.vote_bwd_bounds(bref, dtype, depth, e16)))
    assert set(rat) == {"vote_xyz", "norm", "out", "twin", "dnet"} | ({"dseed"} if bi["dseed"] else set())
    report(dtype, id, rat)


# ---- vote decode, position-major rows -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", IDS(hr.ROWS_CASES))
def test_vote_decode_rows_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    case = hr.case_of(id)
    N, C = case["N"], case["C"]
    inp, bi = hr.rows_case_inputs(case, dtype)
    net, sx, sf = IN(inp["net"]), IN(inp["seed_xyz"]), IN(inp["seed"])
    vx, out, norm = OUT(N, 3, F32), OUT(N, C, dtype), OUT(N, 1, F32)
    rc = lib.omnipq_vote_decode_rows(N, C, P(net), case["ldn"], P(sx), P(sf), P(vx), P(out), P(norm), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(vote_xyz=read(vx, N, 3), norm=read(norm, N, 1).reshape(N), out=read(out, N, C))
    assert intact(net, inp["net"]) and intact(sx, inp["seed_xyz"]) and intact(sf, inp["seed"])
    depth = hr.vote_depth(C, rows=True)
    ref = hr.vote_reference(inp)
    rat = hr.ratios(got, ref, hr.vote_bounds(ref, dtype, depth, True))
    ob, nb, gx, g = IN(bi["out"]), IN(bi["norm"]), IN(bi["g_xyz"]), IN(bi["g"])
    dnet, dseed = OUT(N, case["ldd"], dtype), OUT(N, C, dtype) if bi["dseed"] else None
    rc = lib.omnipq_vote_decode_bwd_rows(N, C, P(ob), P(nb), P(gx), P(g), P(dnet), case["ldd"], P(dseed), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    bgot = dict(dnet=read(dnet, N, case["ldd"]))
    assert zero_bits(bgot["dnet"][:, 3 + C:]), "padding columns are not +0"
    if dseed is not None:
        bgot["dseed"] = read(dseed, N, C)
        assert same_bits(bgot["dseed"], bgot["dnet"][:, 3:3 + C].contiguous()), "dseed and dnet's columns are one rounding"
    assert intact(ob, bi["out"]) and intact(nb, bi["norm"]) and (gx is None or gx.guards_intact()) and (g is None or g.guards_intact())
    bref = hr.vote_bwd_reference(bi)
    bref["dseed"] = bref["dv"]
    rat.update(hr.ratios(bgot, bref, hr.vote_bwd_bounds(bref, dtype, depth, True)))
    assert set(rat) == {"vote_xyz", "norm", "out", "dnet"} | ({"dseed"} if bi["dseed"] else set())
    report(dtype, id, rat)
