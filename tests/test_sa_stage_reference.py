"""CPU: the yardstick of tests/test_gpu_sa_stage_f64.py checked against itself.  tests/sa_stage_reference.py holds a float64
reference of the SA stage's streaming kernels, elementwise bounds, and an emulation of the kernels' arithmetic in f32 / e16 with
their summation shape.  Here: on every case the emulation is finite and inside the bounds (and bit-equal where the reference
says so); every mutant of the emulation is OUTSIDE on a named case; the exactness claim behind the gates (a y + b is exact in
float64 on every case's ranges) is re-checked against fractions.Fraction; rows_per_block / stats_grid as restated in Python
agree with a table written out by hand from csrc/sa_stage.hip; and the two chains (statistics -> finalize, backward statistics
-> apply) stay inside the bounds that propagate e_s1, e_s2 -> e_var -> e_invstd -> e_a, e_b and e_S, e_T -> dY.
"""
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import sa_stage_reference as sr

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
APPLY_SHAPES = [(16, 1), (24, 17), (128, 37), (288, 8), (640, 4)]


def _finite(got):
    return all(bool(torch.isfinite(v.double()).all()) for v in got.values())


# every family: [(case id, evaluate(dtype, mutant) -> (got, ratios, broken))]

def _gather(case):
    def run(dtype, mutant=None):
        inp = sr.gather_inputs(case, dtype)
        got = sr.gather_emulate(inp, dtype, mutant)
        return (got,) + sr.verdict(got, *sr.gather_reference(inp, dtype))
    return run


def _colstats(C, rows, z):
    def run(dtype, mutant=None):
        inp = sr.colstats_inputs(C, rows, dtype, sums0=z)
        got = sr.colstats_emulate(inp, mutant)
        return (got,) + sr.verdict(got, *sr.colstats_reference(inp))
    return run


def _finalize(case):
    def run(dtype, mutant=None):
        inp = sr.finalize_inputs(case)
        got = sr.finalize_emulate(inp, mutant)
        return (got,) + sr.verdict(got, *sr.finalize_reference(inp))
    return run


def _forward(case, op):
    def run(dtype, mutant=None):
        inp = sr.pool_inputs(case, dtype)
        if op == "bnrelu":
            got = sr.bnrelu_emulate(inp, dtype)
            return (got,) + sr.verdict(got, *sr.bnrelu_reference(inp, dtype))
        emu, ref = (sr.pool_emulate, sr.pool_reference) if op == "pool" else (sr.pool_select_emulate, sr.pool_select_reference)
        got = emu(inp, dtype, mutant)
        return (got,) + sr.verdict(got, *ref(inp, dtype, got=got))
    return run


def _stats_inputs(kind, C, rows, dtype):
    return sr.dense_inputs(C, rows, dtype) if kind == "dense" else sr.pool_stats_inputs(C, rows, dtype, select=kind == "sel")


def _bwd_stats(kind, C, rows):
    def run(dtype, mutant=None):
        inp = _stats_inputs(kind, C, rows, dtype)
        got = sr.bwd_stats_emulate(inp, kind, mutant)
        return (got,) + sr.verdict(got, *sr.bwd_stats_reference(inp, kind))
    return run


def _apply(kind, C, rows, form, scale, s=3):
    def run(dtype, mutant=None):
        if kind == "dense":
            inp = sr.dense_inputs(C, rows, dtype)
            positions = rows
        else:
            inp = sr.pool_stats_inputs(C, rows, dtype, select=False, s=s)
            positions = rows * s
        sums = sr.exact_totals(inp, kind, scale)
        got = sr.apply_emulate(inp, kind, sums, scale * positions, dtype, form, mutant)
        return (got,) + sr.verdict(got, *sr.apply_reference(inp, kind, sums, scale * positions, dtype, form))
    return run


def _scatter(case, form):
    def run(dtype, mutant=None):
        inp = sr.scatter_inputs(case, dtype, rows_form=form == "rows")
        got = sr.scatter_emulate(inp, dtype, form, mutant)
        return (got,) + sr.verdict(got, *sr.scatter_reference(inp, dtype, form))
    return run


def _families():
    ev = {}
    for case in sr.GATHER_CASES:
        ev[case["id"]] = _gather(case)
    for C, rows in sr.STATS_SHAPES:
        ev[f"colstats-C{C}-R{rows}"] = _colstats(C, rows, False)
        ev[f"dense-stats-C{C}-R{rows}"] = _bwd_stats("dense", C, rows)
        ev[f"pool-stats-C{C}-R{rows}"] = _bwd_stats("pool", C, rows)
    ev["colstats_z-C24-R17"] = _colstats(24, 17, True)
    for C, rows in sr.SEL_SHAPES:
        ev[f"sel-stats-C{C}-R{rows}"] = _bwd_stats("sel", C, rows)
    for case in sr.FINALIZE_CASES:
        ev[case["id"]] = _finalize(case)
    for case in sr.POOL_CASES:
        for op in ("bnrelu", "pool", "select"):
            ev[f"{op}-{case['id']}"] = _forward(case, op)
        if case["BM"] <= 64:
            ev[f"apply-{case['id']}"] = _apply("pool", case["C"], case["BM"], "pool", 1.0, s=case["s"])
    ev["apply-pool-group"] = _apply("pool", 24, 7, "pool", 2.0, s=5)
    for C, rows in APPLY_SHAPES:
        for form in ("plain", "fused"):
            ev[f"apply-{form}-C{C}-R{rows}"] = _apply("dense", C, rows, form, 1.0)
    ev["apply-fused-group"] = _apply("dense", 24, 17, "fused", 2.0)
    ev["apply-fused-big"] = _apply("dense", sr.BIG_C, sr.BIG_P, "fused", 1.0)
    for case in sr.SCATTER_CASES:
        ev[f"atomic-{case['id']}"] = _scatter(case, "atomic")
        ev[f"csr-{case['id']}"] = _scatter(case, "csr")
    for case in sr.ROWS_CASES:
        ev[case["id"]] = _scatter(case, "rows")
    return ev


FAMILIES = _families()

# mutant -> the case that must catch it
MUTANT_CASE = {
    "rv_biased": "fin-cnt2", "eps_outside": "fin-plain", "rm_no_bias": "fin-plain", "var_unclamped": "fin-plain",
    "gate_ge": "dense-stats-C24-R17", "arg_last": "pool-pool-s5", "select_max_for_neg_a": "select-pool-s5",
    "div_by_P": "apply-pool-group", "T_no_invstd": "dense-stats-C24-R17", "swap_ST": "dense-stats-C24-R17",
    "stats_drop_tail": "colstats-C16-R8193", "bucket_tail_dropped": "csr-scatter-cin8-kpad16",
    "dcentre_plus": "csr-scatter-cin8-kpad16", "dxyz_no_inv_r": "csr-scatter-cin8-kpad16",
    "gather_round_before_scale": "gather-stride", "pad_nonzero": "gather-cin8-kpad16-s4",
}
# the same defect seen through another kernel
MUTANT_ALSO = [("gate_ge", "apply-fused-C24-R17"), ("gate_ge", "apply-plain-C24-R17"), ("div_by_P", "apply-fused-group"),
               ("stats_drop_tail", "sel-stats-C640-R1537"), ("stats_drop_tail", "dense-stats-C288-R3585"),
               ("bucket_tail_dropped", "rows-C16"), ("dcentre_plus", "rows-C16"), ("swap_ST", "sel-stats-C16-R17")]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("id", sorted(FAMILIES))
def test_the_emulation_is_finite_and_inside_the_bounds(id, dtype):
    got, rat, broken = FAMILIES[id](dtype)
    assert _finite(got), id
    assert not broken, (id, broken, sr.fmt(rat))


def test_there_are_sixteen_mutants():
    assert len(MUTANT_CASE) == 16 and all(case in FAMILIES for case in MUTANT_CASE.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mutant,id", sorted(MUTANT_CASE.items()) + MUTANT_ALSO)
def test_every_mutant_is_caught_on_its_case(mutant, id, dtype):
    _, rat, broken = FAMILIES[id](dtype, mutant)
    print(f"\n  MUTANT {mutant} caught on {id}: {broken}")
    assert broken, (mutant, id, sr.fmt(rat))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_y_plus_b_is_exact_in_float64_on_every_case(dtype):
    checked = 0
    for case in sr.POOL_CASES:
        inp = sr.pool_inputs(case, dtype)
        assert sr.in_exact_ranges(inp["a"], inp["b"], inp["Y"])
        assert sr.fraction_mismatches(inp["a"], inp["b"], inp["Y"], samples=100) == 0, case["id"]
        checked += 1
    for C, rows in sr.STATS_SHAPES + APPLY_SHAPES:
        inp = sr.dense_inputs(C, rows, dtype)
        assert sr.in_exact_ranges(inp["a"], inp["b"], inp["Y"])
        assert sr.fraction_mismatches(inp["a"], inp["b"], inp["Y"], samples=100) == 0, (C, rows)
        checked += 1
    assert checked == len(sr.POOL_CASES) + len(sr.STATS_SHAPES) + len(APPLY_SHAPES)
    # and the range itself: random triples at the edges of the three ranges
    gen = torch.Generator().manual_seed(1)
    n = 2000
    a = (sr.dy(gen, (n,), -3, 2) * 2.0 ** torch.randint(-3, 3, (n,), generator=gen)).clamp(-4, 4)
    a = torch.sign(a) * a.abs().clamp(2.0 ** -3, 4.0)
    b = torch.sign(a) * sr.dy(gen, (n,), -6, 2, 0.3).abs()
    y = sr.dy(gen, (1, n), -6, 3, 3.0).to(dtype)
    assert sr.in_exact_ranges(a, b, y) and sr.fraction_mismatches(a, -b, y, samples=n) == 0


def test_launch_geometry_against_the_c_source():
    # rows_per_block: min(16, 256 / (C / 8)); written out by hand
    assert [sr.rows_per_block(C) for C in (16, 24, 128, 136, 256, 288, 512, 640)] == [16, 16, 16, 15, 8, 7, 4, 3]
    # stats_grid(rows, C): ceil(rows / rpb) up to 512 blocks; beyond, ceil(blocks / 512) <= 32 rows per lane; at most 1024
    table = {(1, 16): 1, (16, 16): 1, (17, 16): 2, (8192, 16): 512, (8193, 16): 257, (1537, 640): 257, (3585, 288): 257,
             (0, 16): 1, (10 ** 7, 16): 1024, (1536, 640): 512, (16 * 512 * 32, 16): 512, (16 * 512 * 32 + 1, 16): 513}
    for (rows, C), blocks in table.items():
        assert sr.stats_grid(rows, C) == blocks, (rows, C)
    assert sr.chain(8193, 16) == (257, 16, 2, 16) and sr.chain(8193, 16, sel=True) == (128, 16, 5, 19)
    assert sr.chain(1, 640) == (1, 3, 1, 0) and sr.chain(2, 640) == (1, 3, 1, 1)
    assert sr.sel_step(16) == 2048 and sr.sel_step(288) == 896 and sr.sel_step(640) == 384
    for C in sr.WIDTHS:                                      # the case table walks both sides of every step
        rpb = sr.rows_per_block(C)
        assert sr.chain(512 * rpb + 1, C)[2] == 2 and sr.chain(rpb + 1, C)[0] == 2
        assert [sr.chain(r, C, sel=True)[2] for r in (sr.sel_step(C) + 1, 3 * sr.sel_step(C) + 5, 4 * sr.sel_step(C) + 1)] == [2, 4, 5]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,rows", [(24, 17), (288, 3585), (16, 15)])
def test_forward_chain_stays_inside_the_propagated_bounds(C, rows, dtype):
    """statistics -> finalize, the emulated totals fed on; the reference takes the EXACT totals and e_s1, e_s2"""
    inp = sr.colstats_inputs(C, rows, dtype)
    want, bnd, _ = sr.colstats_reference(inp)
    gen = torch.Generator().manual_seed(C + rows)
    fin = dict(cnt=float(rows), gamma=torch.randn(C, generator=gen), beta=torch.randn(C, generator=gen), eps=sr.as_f32(sr.EPS),
               mom=sr.as_f32(0.1), rm=torch.randn(C, generator=gen), rv=torch.rand(C, generator=gen) + 0.5, bias=None)
    got = sr.finalize_emulate(dict(fin, sums=sr.colstats_emulate(inp)["sums"]))
    ref = sr.finalize_reference(dict(fin, sums=want["sums"]), e_s1=bnd["sums"][0] / sr.MARGIN, e_s2=bnd["sums"][1] / sr.MARGIN)
    rat, broken = sr.verdict(got, *ref)
    assert _finite(got) and not broken, (broken, sr.fmt(rat))
    # the large-mean channel is where e_var is felt: its bound on invstd is well above one f32 rounding
    assert float(ref[1]["invstd"][7] / ref[0]["invstd"][7]) > 4 * sr.MARGIN * sr.U32 or rows < 100


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form,C,rows", [("fused", 24, 17), ("plain", 288, 3585), ("fused", 16, 8193), ("pool", 24, 17)])
def test_backward_chain_stays_inside_the_propagated_bounds(form, C, rows, dtype):
    kind = "pool" if form == "pool" else "dense"
    inp = _stats_inputs(kind, C, rows, dtype)
    positions = rows * (3 if kind == "pool" else 1)
    want, bnd, _ = sr.bwd_stats_reference(inp, kind)
    got = sr.apply_emulate(inp, kind, sr.bwd_stats_emulate(inp, kind)["sums"], float(positions), dtype, form)
    ref = sr.apply_reference(inp, kind, want["sums"], float(positions), dtype, form, e_S=bnd["sums"][0] / sr.MARGIN,
                             e_T=bnd["sums"][1] / sr.MARGIN)
    got.pop("gb")                                            # (the f32 copy is of the emulated totals, not of the exact ones)
    rat, broken = sr.verdict(got, *ref)
    assert _finite(got) and not broken, (broken, sr.fmt(rat))


def test_hot_words_are_the_rounded_product_over_the_row():
    inp = sr.pool_stats_inputs(24, 17, torch.bfloat16, select=True)
    hot = sr.hot_words(inp, torch.bfloat16)
    assert hot.dtype is torch.int32 and bool(((hot & 0xFF) == inp["arg"].to(torch.int32)).all())
    live = inp["out_pm"].double() > 0
    assert bool(live.any()) and bool((~live).any())
    assert bool((((hot >> 16) & 0x7FFF)[~live] == 0).all())                     # a * 0: +-0
