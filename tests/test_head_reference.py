"""CPU: the float64 reference of the head and vote decode kernels and its elementwise bounds (tests/head_reference.py) have teeth.

On every case the GPU suite runs (tests/test_gpu_head_f64.py walks the same tables), a torch-CPU emulation of the kernels' f32
arithmetic in their order stays inside every bound, at or below 1 / MARGIN of it, and each of thirteen plausible kernel defects
put into that emulation leaves a bound (or fails the norm's round trip) on the case named for it.

Largest error / bound ratio of the emulation per output over all cases (bfloat16 | half), measured:
    object head  center 0.666 | 0.666   hr  0.616 | 0.648   sr  0.666 | 0.664   pred  0.620 | 0.620   dy  0.663 | 0.661
                 dbase  0.646 | 0.646
    quad head    norm   0.609 | 0.578   center 0.667 | 0.667   normal 0.594 | 0.562   dy  0.661 | 0.662   dbase  0.667 | 0.667
    vote         vote_xyz 0.666 | 0.666   norm 0.156 | 0.183   out  0.662 | 0.661   twin  0.664 | 0.662
                 dnet   0.664 | 0.663   dseed  0.663 | 0.663
    vote rows    vote_xyz 0.662 | 0.663   norm 0.101 | 0.130   out  0.663 | 0.660   dnet  0.663 | 0.661   dseed  0.663 | 0.661
A single f32 operation or an e16 store at its worst rounding sits at 1 / MARGIN of its bound (u32 and u are unit roundoffs);
every case is asserted to stay at or below 1 / MARGIN.
"""
import os
import re

import pytest
import torch

import head_reference as hr

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
IDS = lambda cases: [c["id"] for c in cases]                                   # noqa: E731


def bits_equal(got, ref, names):
    return all(torch.equal(got[n].view(torch.int16), ref[n].view(torch.int16)) for n in names)


def run_head(case, dtype, mutant=None):
    inp, grads = hr.head_case_inputs(case, dtype)
    prior = hr.dbase_prior(case, case["B"] * case["K"])
    ref = hr.head_reference(inp)
    got = hr.head_emulate(inp, dtype, mutant)
    assert bits_equal(got, ref, hr.HEAD_BITS)
    rat = hr.ratios({n: got[n] for n in hr.HEAD_BOUNDED}, ref, hr.head_bounds(ref, dtype))
    bref = hr.head_bwd_reference(inp, grads, case["lddy"], prior)
    bgot = hr.head_bwd_emulate(inp, grads, case["lddy"], prior, dtype, mutant)
    rat.update(hr.ratios(bgot, bref, hr.head_bwd_bounds(bref, dtype)))
    return rat


def run_quad(case, dtype, mutant=None):
    inp, grads = hr.quad_case_inputs(case, dtype)
    prior = hr.dbase_prior(case, case["R"])
    ref = hr.quad_reference(inp)
    got = hr.quad_emulate(inp, dtype, mutant)
    assert bits_equal(got, ref, ("scores", "size"))
    rat = hr.ratios({n: got[n] for n in ("norm", "center", "normal")}, ref, hr.quad_bounds(ref, dtype))
    norm_in = hr.quad_case_norm(case, inp, dtype)
    bref = hr.quad_bwd_reference(inp, grads, case["lddy"], norm_in, prior)
    bgot = hr.quad_bwd_emulate(inp, grads, case["lddy"], norm_in, prior, dtype, mutant)
    rat.update(hr.ratios(bgot, bref, hr.quad_bwd_bounds(bref, dtype)))
    return rat, hr.norm_round_trips(got["norm"], dtype)


def run_vote(case, dtype, mutant=None):
    rows = "N" in case
    if rows:
        inp, bi = hr.rows_case_inputs(case, dtype)
        e16 = True
    else:
        inp, bi, ft = hr.vote_case_inputs(case, dtype)
        e16 = ft is not torch.float32
    depth = hr.vote_depth(case["C"], rows)
    ref = hr.vote_reference(inp)
    rat = hr.ratios(hr.vote_emulate(inp, dtype, rows, e16, mutant), ref | dict(twin=ref["out"]), hr.vote_bounds(ref, dtype, depth, e16))
    bref = hr.vote_bwd_reference(bi)
    bref["dseed"] = bref["dv"]
    rat.update(hr.ratios(hr.vote_bwd_emulate(bi, dtype, rows, e16, mutant), bref, hr.vote_bwd_bounds(bref, dtype, depth, e16)))
    return rat


def run(case, dtype, mutant=None):
    if case["id"].startswith("head"):
        return run_head(case, dtype, mutant)
    if case["id"].startswith("quad"):
        return run_quad(case, dtype, mutant)[0]
    return run_vote(case, dtype, mutant)


def test_case_table_covers_what_it_says():
    ids = IDS(hr.ALL_CASES)
    assert len(set(ids)) == len(ids)
    hs = hr.HEAD_CASES
    dims = {(1, 18, 18): 97, (12, 10, 10): 79, (1, 1, 1): 12, (12, 18, 37): 138}
    assert {c["dims"] for c in hs} == set(dims) and all(hr.head_width(*d) == w for d, w in dims.items())
    for d, w in dims.items():
        mine = [c for c in hs if c["dims"] == d]
        assert {(c["B"], c["K"]) for c in mine} == {(1, 1), (1, 2), (3, 1), (2, 5), (3, 85)}
        assert {c["ldy"] for c in mine} == {w, (w + 7) // 8 * 8, (w + 7) // 8 * 8 + 8}
        assert {c["lddy"] for c in mine} == {w, w + 3, w + 130}
        assert {c["score"] for c in mine} == set(hr.SCORE_KINDS) == {"random", "tie", "equal", "last", "zeros"}
        assert {c["rot"] for c in mine} == {0, 1, 2, 3, 4}                         # every output meets every kind
        assert {c["dbase"] for c in mine} == set(hr.DBASE_KINDS) == {"null", "fresh", "acc"}
    assert set(hr.GRAD_KINDS) == {"e16", "f32", "null", "scalar", "view"}
    for i in range(10):
        assert {hr.rotated_kinds(rot, 10)[i] for rot in range(5)} == set(hr.GRAD_KINDS)
    assert max(dims.values()) > 128 and any(c["lddy"] - 138 > 128 for c in hs if c["dims"] == (12, 18, 37))   # both second trips
    qs = hr.QUAD_CASES
    assert {c["R"] for c in qs} == {1, 31, 32, 33, 255, 257, 1023, 1025, 1281, 2304} and all(c["B"] * c["K"] == c["R"] for c in qs)
    assert {(c["B"], c["K"]) for c in qs if c["R"] == 1281} == {(3, 427)}
    assert {c["B"] == 1 for c in qs if c["R"] > 1} == {True, False}
    assert {c["ldy"] for c in qs} == {10, 32} and {c["lddy"] for c in qs} == {10, 16, 35}
    assert {c["rot"] for c in qs} == {0, 1, 2, 3, 4} and {c["dbase"] for c in qs} == set(hr.DBASE_KINDS)
    assert {c["norm"] for c in qs} == {"own", "any"}
    for R in hr.QUAD_RS:
        assert {c["kind"] for c in qs if c["R"] == R} == set(hr.QUAD_KINDS) == {"randn", "dominated", "offset"}
        assert {c["lddy"] for c in qs if c["R"] == R} == {10, 16, 35}
    assert [(c["B"] * c["Kh"], c["B"] * c["Kq"]) for c in hr.PAIR_CASES] == [(3, 33), (170, 1281)]
    assert hr.GROUP_CASE["n"] == 5
    vs = hr.VOTE_CASES
    assert {(c["B"], c["K"]) for c in vs} == {(1, 1), (2, 31), (1, 32), (3, 33), (2, 77)}
    for C in (1, 8, 67, 288, 320):
        mine = [c for c in vs if c["C"] == C]
        assert len(mine) == 5 and {c["ld"] % 8 == 0 for c in mine} == {True, False} == {c["ldd"] % 8 == 0 for c in mine}
        assert all(c["ld"] >= C + 3 and c["ldd"] >= C + 3 for c in mine)
    assert {c["layout"] for c in vs} == set(hr.VOTE_LAYOUTS) and {c["null"] for c in vs} == set(hr.VOTE_NULLS)
    assert {(c["layout"], c["ld"] % 8 == 0) for c in vs} == {(lay, by8) for lay in hr.VOTE_LAYOUTS for by8 in (True, False)}
    rs = hr.ROWS_CASES
    assert {c["N"] for c in rs} == {1, 3, 4, 5, 131} and {c["C"] for c in rs} == {8, 288, 320} and len(rs) == 15
    for C in (8, 288, 320):
        assert {c["ldn"] for c in rs if c["C"] == C} == {C + 8, C + 16} == {c["ldd"] for c in rs if c["C"] == C}
    assert any(c["C"] == 320 and c["ldd"] == 336 for c in rs) and any(c["C"] == 320 and c["ldn"] == 336 for c in rs)
    assert {c["null"] for c in rs} == set(hr.VOTE_NULLS)
    assert max(c["B"] * c["K"] for c in hs + qs + vs) <= 2304                       # tiny: a few thousand rows at the most


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_inputs_are_what_their_kind_promises(dtype):
    for c in hr.HEAD_CASES:
        inp, grads = hr.head_case_inputs(c, dtype)
        ns, w = c["dims"][1], hr.head_width(*c["dims"])
        s = hr._part(inp, "ss").double()
        pick = hr.first_max(inp)
        top = (s == s.max(dim=1, keepdim=True).values).sum(dim=1)
        if c["score"] == "tie":
            assert bool((pick == 0).all()) and bool((top == min(ns, 2)).all()) and bool((s[:, ns - 1] == s[:, 0]).all())
        elif c["score"] == "equal":
            assert bool((pick == 0).all()) and bool((top == ns).all())
        elif c["score"] == "last":
            assert bool((pick == ns - 1).all()) and bool((top == 1).all())
        elif c["score"] == "zeros":
            sb = hr._part(inp, "ss").view(torch.int16)
            assert bool((pick == 0).all()) and bool((sb[:, ns - 1] == 0).all()) and (ns == 1 or bool((sb[:, 0] == -32768).all()))
        assert bool(torch.isnan(inp["y"][:, w:].float()).all()) and bool(torch.isfinite(inp["y"][:, :w].float()).all())
        assert [g.kind for g in grads] == hr.rotated_kinds(c["rot"], 10)
    inp, _ = hr.quad_case_inputs(hr.case_of("quad-R1025-dominated"), dtype)
    sq = inp["y"][:, 5:8].double().pow(2).sum(dim=1)
    assert float(sq[[0, 512, 1024]].sum() / sq.sum()) > 0.99 and float(sq[1024] / sq.sum()) > 0.05
    inp, _ = hr.quad_case_inputs(hr.case_of("quad-R257-offset"), dtype)
    assert float((inp["y"][:, 5:8].double() - 5.0).abs().max()) < 0.125


def test_descriptor_addressing_agrees_with_torch_views():
    """grad_values is index arithmetic; torch's as_strided is the other statement of the same layout"""
    gen = torch.Generator().manual_seed(1)
    B, K, n1 = 3, 4, 5
    for n2 in (1, 3):
        for kind in ("e16", "f32", "scalar", "view"):
            g = hr.make_grad(gen, B, K, n1, n2, kind, torch.bfloat16, alt=False)
            want = torch.as_strided(g.storage, (B, K, n1, n2), (g.sb, g.sk, g.s1, g.s2)).double().reshape(B * K, n1 * n2)
            assert torch.equal(hr.grad_values(g, B, K, n1 * n2), want)
        v = hr.make_grad(gen, B, K, n1, n2, "view", torch.bfloat16, alt=True)
        assert v.storage.dtype is torch.bfloat16 and (v.sb, v.sk, v.s1, v.s2) == (n2 * n1 * K, 1, K, n1 * K)
    assert not bool(hr.grad_values(hr.make_grad(gen, B, K, n1, 1, "null", torch.bfloat16, False), B, K, n1).any())


def test_reference_agrees_with_autograd():
    """the closed-form backward of each reference is the derivative of its forward"""
    dt = torch.bfloat16
    c = hr.case_of("head-w97-1x2-tie-rot1")
    inp, grads = hr.head_case_inputs(c, dt)
    w = hr.head_width(*c["dims"])
    g = [hr.grad_values(x, c["B"], c["K"], wd) for x, wd in zip(grads, hr.head_out_widths(*c["dims"]))]
    y = inp["y"][:, :w].double().requires_grad_(True)
    base = inp["base"].double().requires_grad_(True)
    col, ns = hr.head_cols(*c["dims"]), c["dims"][1]
    part = lambda n: y[:, col[n][0]:col[n][0] + col[n][1]]                     # noqa: E731
    means = inp["means"].double().reshape(1, 3 * ns)
    sr = part("srn") * means
    pred = torch.gather(sr + means, 1, 3 * hr.first_max(inp)[:, None] + torch.arange(3)[None, :])
    outs = [part("obj"), part("ctr") + base, part("hs"), part("hrn"), part("hrn") * inp["hr_scale"], part("ss"), part("srn"), sr,
            pred, part("sem")]
    dy, db = torch.autograd.grad(outs, [y, base], g)
    ref = hr.head_bwd_reference(inp, grads, w, None)
    assert float((dy - ref["dy"]).abs().max()) < 1e-12 and float((db - ref["dbase"]).abs().max()) < 1e-12
    c = hr.case_of("quad-R33-randn")
    inp, grads = hr.quad_case_inputs(c, dt)
    g = [hr.grad_values(x, c["B"], c["K"], wd) for x, wd in zip(grads, hr.QUAD_WIDTHS)]
    y = inp["y"][:, :10].double().requires_grad_(True)
    nrm = y[:, 5:8].norm()
    dy, = torch.autograd.grad([y[:, 0:2], y[:, 2:5] + inp["base"].double(), y[:, 5:8] / nrm, y[:, 8:10]], [y], g)
    ref = hr.quad_bwd_reference(inp, grads, 10, float(nrm.detach()), None)
    assert float((dy - ref["dy"]).abs().max()) < 1e-6 * float(dy.abs().max())      # norm_in is the f32 rounding of nrm
    c = hr.case_of("vote-3x33-C67")
    inp, bi, _ = hr.vote_case_inputs(c, dt)
    C = c["C"]
    net, seed = inp["net"][:, :3 + C].double().requires_grad_(True), inp["seed"].double().requires_grad_(True)
    v = seed + net[:, 3:]
    out = v / v.norm(dim=1, keepdim=True)
    gx, gf = torch.randn(out.shape[0], 3, dtype=torch.float64), torch.randn(out.shape, dtype=torch.float64)
    dn, ds = torch.autograd.grad([inp["seed_xyz"].double() + net[:, :3], out], [net, seed], [gx, gf])
    ref = hr.vote_bwd_reference(dict(out=out.detach(), norm=v.detach().norm(dim=1), g_xyz=gx, g=gf, ldd=C + 3))
    assert float((dn - ref["dnet"]).abs().max()) < 1e-12 and float((ds - ref["dv"]).abs().max()) < 1e-12


# the margin of 1.5 is for what the emulation does not do (contraction, the hardware's division and sqrt): the emulation
# itself must not need it
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("id", IDS(hr.ALL_CASES))
def test_emulated_kernel_arithmetic_is_inside_every_bound(id, dtype):
    c = hr.case_of(id)
    rat = run(c, dtype)
    print(f"\n  RATIO emulation {dtype} {id}: {hr.fmt(rat)}")
    if id.startswith("head"):
        assert set(rat) == set(hr.HEAD_BOUNDED) | {"dy", "dbase"}
    elif id.startswith("quad"):
        assert set(rat) == {"norm", "center", "normal", "dy", "dbase"}
        assert run_quad(c, dtype)[1], "the norm is no e16 number"
    else:
        assert set(rat) == {"vote_xyz", "norm", "out", "twin", "dnet", "dseed"}
    assert not hr.outside(rat), (id, hr.fmt(rat))
    assert max(r[0] for r in rat.values()) <= 1.0 / hr.MARGIN, (id, hr.fmt(rat))


MUTANT_CASES = [
    ("argmax_last", "head-w97-1x2-tie-rot1", "pred"),                   # the last maximum of a tie
    ("argmax_last", "head-w79-3x1-zeros-rot3", "pred"),                 # ... and +0 taken for larger than -0
    ("hr_scale_on_hrn", "head-w79-1x1-equal-rot1", "dy"),               # hr_scale on g_hrn instead of g_hr
    ("pred_no_means", "head-w97-1x1-random-rot0", "dy"),                # g_pred added behind the product with means
    ("pred_pick_minus_1", "head-w97-1x1-random-rot0", "dy"),            # g_pred routed to the cluster in front
    ("dy_pad_unwritten", "head-w138-3x1-last-rot0", "dy"),              # lddy = width + 130: both trips of the zero fill
    ("dbase_replace", "head-w97-3x1-equal-rot2", "dbase"),              # accumulate stores instead of adding
    ("quad_drop_rows_ge_1024", "quad-R1025-dominated", "norm"),         # row 1024 carries a third of the sum
    ("quad_drop_rows_ge_1024", "quad-R2304-randn", "normal"),
    ("quad_count_clamped", "quad-R257-randn", "norm"),                  # the partly filled quartet
    ("quad_count_clamped", "quad-R1025-dominated", "norm"),             # the clamp of the second trip: row 1024 four times
    ("n2_for_n3", "quad-R33-randn", "dy"),
    ("dy_pad_unwritten", "quad-R33-offset", "dy"),
    ("dbase_replace", "quad-R31-offset", "dbase"),
    ("vote_dot_wrong_point", "vote-3x33-C67", "dnet"),
    ("vote_no_projection", "vote-2x31-C8", "dseed"),
    ("vote_no_projection", "rows-131-C288", "dnet"),
    ("rows_ignore_last_lane", "rows-5-C8", "norm"),
    ("rows_ignore_last_lane", "rows-131-C288", "dnet"),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mutant,id,where", MUTANT_CASES)
def test_mutant_leaves_a_bound(mutant, id, where, dtype):
    assert {m for m, _, _ in MUTANT_CASES} | {"norm_not_rounded"} == set(hr.MUTANTS)
    assert not hr.outside(run(hr.case_of(id), dtype))
    bad = hr.outside(run(hr.case_of(id), dtype, mutant))
    assert where in bad, (mutant, id, bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_unrounded_norm_fails_the_round_trip(dtype):
    """inside every bound (the bound allows the rounding, it cannot demand it): the round trip is what sees it"""
    for id in ("quad-R33-randn", "quad-R1281-offset"):
        rat, trips = run_quad(hr.case_of(id), dtype, "norm_not_rounded")
        assert not trips and "norm" not in hr.outside(rat), id
        assert run_quad(hr.case_of(id), dtype)[1]


def test_one_wrong_row_is_seen():
    """what a norm ratio at 2 % hides: one row of 255 with its pred gradient in the neighbouring cluster"""
    c = hr.case_of("head-w138-3x85-random-rot2")
    dt = torch.bfloat16
    inp, grads = hr.head_case_inputs(c, dt)
    ref = hr.head_bwd_reference(inp, grads, c["lddy"], hr.dbase_prior(c, 255))
    good = hr.head_bwd_emulate(inp, grads, c["lddy"], hr.dbase_prior(c, 255), dt)
    bad = hr.head_bwd_emulate(inp, grads, c["lddy"], hr.dbase_prior(c, 255), dt, "pred_pick_minus_1")
    got = dict(dy=good["dy"].clone())
    got["dy"][254] = bad["dy"][254]
    rel = float((got["dy"].double() - ref["dy"]).norm() / ref["dy"].norm())
    assert 0 < rel < 2e-2
    out = hr.outside(hr.ratios(got, ref, hr.head_bwd_bounds(ref, dt)))
    assert set(out) == {"dy"} and 1 <= out["dy"][1] <= 6, out


def test_gpu_suite_calls_every_entry_point_of_head_ops():
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "omni-pq_amd", "csrc", "head_ops.hip")).read()
    names = set(re.findall(r'extern "C" int (omnipq_\w+)\(', src))
    gpu = open(os.path.join(here, "test_gpu_head_f64.py")).read()
    assert len(names) == 12 and not {n for n in names if f"lib.{n}(" not in gpu}
