"""CPU: the float64 reference of the decoder's row kernels and its elementwise bounds (tests/decoder_reference.py) have teeth.

On every case the GPU suite runs (tests/test_gpu_decoder_f64.py walks the same tables), a torch-CPU emulation of the
kernels' f32 arithmetic in their order stays inside every bound, and each of eleven plausible kernel defects put into that
emulation leaves at least one bound on the case named for it.  The dropout mask is the restated hash here as on the GPU.

Largest error / bound ratio of the emulation per output over all LayerNorm cases (bfloat16 | half), measured:
    mean  0.126 | 0.118    rstd    0.216 | 0.222    out32  0.312 | 0.469    out16  0.664 | 0.664
    dx    0.181 | 0.181    out_pe  0.664 | 0.665    dy     0.663 | 0.662    dgb    0.186 | 0.186
The e16 outputs sit at one store rounding (1 / MARGIN of the bound when the rounding is at its worst); every case is
asserted to stay at or below 1 / MARGIN.
"""
import math

import pytest
import torch

import decoder_reference as dr

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]


def run(case, dtype, mutant=None):
    inp = dr.case_inputs(case, dtype)
    keep = dr.case_mask(case)
    got = dr.emulate(inp, keep, case["p"], dtype, mutant=mutant)
    ref = dr.reference(inp, keep, case["p"])
    return dr.ln_ratios(got, ref, dr.bounds(ref, dtype, "atomic"))


def expected_outputs(case):
    return set(dr.LN_OUTPUTS) - (set() if case["y"] else {"dy"}) - (set() if case["outs"] == "pe" else {"out_pe"})


def test_case_table_covers_what_it_says():
    ids = dr.CASE_IDS
    assert len(set(ids)) == len(ids)
    cs = dr.CASES
    assert {c["C"] for c in cs if c["id"].startswith("C-")} == {4, 8, 252, 256, 260, 288, 512, 516, 768, 772, 1020, 1024}
    assert all(c["R"] == 5 for c in cs if c["id"].startswith("C-"))
    assert {c["R"] for c in cs if c["id"].startswith("R-")} == {1, 3, 4, 5, 37}
    assert all(c["C"] == 260 for c in cs if c["id"].startswith("R-"))
    fwd, bwd = dr.case_of("stride-fwd"), dr.case_of("stride-bwd")
    assert (fwd["R"], fwd["C"]) == (8192 + 5, 8) and fwd["R"] > 2048 * 4           # rows_grid(): at most 2048 blocks
    assert (bwd["R"], bwd["C"]) == (2048 + 5, 260) and bwd["R"] > dr.ln_blocks(bwd["R"]) * 4 and dr.ln_blocks(bwd["R"]) == 512
    assert {c["kind"] for c in cs} == set(dr.KINDS) == {"randn", "offset", "tiny", "constant", "mixed"}
    assert {c["gamma"] for c in cs} == {"plain", "signed"}
    assert {c["y"] for c in cs} == {True, False}
    assert {c["p"] for c in cs if c["y"]} == {0.0, 0.1, 0.5, 1e-12, 0.9}
    assert {c["outs"] for c in cs} == {"32", "16", "both", "pe"}
    assert {c["grads"] for c in cs} == {"g32", "g16", "gpe", "all", "none"}
    assert {c["route"] for c in cs} == {"atomic", "partials"}
    assert {c["route"] for c in cs if c["R"] == 2053} == {"atomic", "partials"}
    assert all(c["C"] % 4 == 0 and 4 <= c["C"] <= 1024 for c in cs)
    assert max(c["R"] * c["C"] for c in cs) <= 2053 * 260                          # small: a few seconds each at the most
    assert set(dr.REDUCE_BLOCKS) == {1, 2, 3, 4, 5, 12, 13, 16, 17, 512}
    items = dr.reduce_items()
    assert len(items) == 32 and {C for _, C in items} >= {4, 1024} and len({b for b, _ in items}) >= 8
    assert dr.FLAT_NS[0] == 4 and dr.FLAT_NS[-1] == 4096 * 256 * 4 + 4
    assert dr.ADDN_NS[0] == 8 and dr.ADDN_NS[-1] == 2048 * 256 * 8 + 8 and set(dr.ADDN_COUNTS) == {1, 2, 5, 16}
    assert {c["cin"] for c in dr.PAD_CASES} >= {0, 3} and any(c["cin"] == c["k"] for c in dr.PAD_CASES)
    assert all(c["ldx"] > c["cin"] for c in dr.PAD_CASES)
    assert {c["c"] for c in dr.SPLIT_CASES} == {8, 288}
    assert {(c["p0"] == 0, c["p0"] == 1, c["p0"] == c["p"] - 1, c["p0"] == c["p"]) for c in dr.SPLIT_CASES if c["p"] == 7} == \
        {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_inputs_are_what_their_kind_promises(dtype):
    def ref_of(id):
        c = dr.case_of(id)
        return dr.reference(dr.case_inputs(c, dtype), dr.case_mask(c), c["p"])

    for id in ("kind-offset", "kind-offset-1024"):
        r = ref_of(id)
        assert float((r["mu"].abs() / r["var"].sqrt()).min()) > dr.OFFSET_RATIO
        assert 0.5 < float(r["var"].min()) and float(r["var"].max()) < 3.0
    r = ref_of("kind-tiny")
    assert float(r["var"].max()) < 0.5 * r["eps"] and float(r["var"].min()) > 0.01 * r["eps"]     # eps decides rstd
    for id in ("kind-constant", "kind-constant-noy"):
        r = ref_of(id)
        assert float((r["var"].sqrt() / r["mu"].abs()).max()) < 1e-15                           # zero but for float64's own sum
        assert float((r["rstd"] - r["eps"] ** -0.5).abs().max()) < 1e-9
        assert float(r["mu"].abs().min()) > 1e-3
    r = ref_of("kind-mixed")
    assert bool(((r["r"].abs() > 250).sum(dim=1) == 1).all())
    g = dr.case_inputs(dr.case_of("gamma-signed"), dtype)["gamma"]
    assert int((g == 0).sum()) >= 288 // 3 and int((g < 0).sum()) > 50 and int((g > 0).sum()) > 50
    inp = dr.case_inputs(dr.case_of("grads-none"), dtype)
    assert inp["g32"] is None and inp["g16"] is None and inp["gpe"] is None
    assert dr.case_inputs(dr.case_of("y-null"), dtype)["y"] is None
    h = dr.flat_inputs(4096, dtype, 0)
    sub = float(torch.finfo(dtype).tiny)
    assert int(((h.double().abs() > 0) & (h.double().abs() < sub)).sum()) >= 4                  # subnormals
    assert int((h.view(torch.int16) == -32768).sum()) >= 2                                      # -0
    h4 = dr.flat_inputs(4, dtype, 0)
    assert h4.double().tolist()[:2] == [0.0, -0.0] and 0 < float(h4[2]) < sub


def test_reference_agrees_with_autograd():
    """the closed-form backward of the reference is the derivative of its forward"""
    c = dr.case_of("gamma-signed")
    inp = dr.case_inputs(c, torch.bfloat16)
    keep = dr.case_mask(c)
    x, y, gamma, beta = (inp[n].double().requires_grad_(True) for n in ("x", "y", "gamma", "beta"))
    p = dr.as_f32(c["p"])
    r = x + keep.double() * y / (1 - p)
    out = torch.nn.functional.layer_norm(r, (c["C"],), gamma, beta, dr.as_f32(dr.EPS))
    t = inp["g32"].double() + inp["g16"].double() + inp["gpe"].double()
    dx, dy, dg, db = torch.autograd.grad(out, [x, y, gamma, beta], t)
    ref = dr.reference(inp, keep, c["p"])
    acc0 = inp["acc0"].double()
    for a, b in ((out, ref["out32"]), (dx, ref["dx"]), (dy, ref["dy"]), (torch.cat([dg, db]), ref["dgb"] - acc0)):
        assert float((a.detach() - b).abs().max()) <= 1e-12 * float(b.abs().max())


# the margin of 1.5 is for what the emulation does not do (fused multiply-adds, the hardware's rsqrt, atomics in another
# order): the emulation itself must not need it
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("id", dr.CASE_IDS)
def test_emulated_kernel_arithmetic_is_inside_every_bound(id, dtype):
    c = dr.case_of(id)
    rat = run(c, dtype)
    print(f"\n  RATIO emulation {dtype} {id}: {dr.fmt(rat)}")
    assert set(rat) == expected_outputs(c)
    assert not dr.outside(rat), (id, dr.fmt(rat))
    assert max(r[0] for r in rat.values()) <= 1.0 / dr.MARGIN, (id, dr.fmt(rat))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_partials_route_sums_to_the_reference(dtype):
    for id in ("R-5", "R-37", "stride-bwd-partials"):
        c = dr.case_of(id)
        inp, keep = dr.case_inputs(c, dtype), dr.case_mask(c)
        got = dr.emulate(inp, keep, c["p"], dtype)
        ref = dr.reference(inp, keep, c["p"])
        assert got["part"].shape == (dr.ln_blocks(c["R"]), 2 * c["C"])
        rat = dr.ratios(dict(dgb=got["part"].double().sum(dim=0)), ref, dr.bounds(ref, dtype, "partials"))
        assert not dr.outside(rat) and rat["dgb"][0] <= 1.0 / dr.MARGIN, (id, rat)


LN_MUTANT_CASES = [
    ("one_pass_var", "kind-offset", "rstd"),            # E[r^2] - mu^2 at |mu| / sigma ~ 1e3
    ("padded_divisor", "C-260", "mean"),                # sums divided by 512
    ("eps_after_sqrt", "kind-tiny", "rstd"),            # 1 / (sqrt(var) + eps)
    ("no_m2", "C-288", "dx"),                           # dx without xh mean(go xh)
    ("dy_no_scale", "p-0.5", "dy"),                     # dy = keep dx
    ("mask_padded_pitch", "C-260", "out32"),            # mask index row * 512 + c
    ("dgb_drop_tail_rows", "R-5", "dgb"),               # the last R % 4 rows missing from dgamma / dbeta
    ("pe_double_rounding", "C-288", "out_pe"),          # out_pe from the rounded out16
    ("bwd_g32_only", "grads-all", "dx"),                # g16 / g16_pe ignored when g32 is given
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mutant,id,where", LN_MUTANT_CASES)
def test_mutant_leaves_a_bound(mutant, id, where, dtype):
    assert {m for m, _, _ in LN_MUTANT_CASES} | {"reduce_no_tail", "relu_gate_from_grad"} == set(dr.MUTANTS)
    assert not dr.outside(run(dr.case_of(id), dtype))
    bad = dr.outside(run(dr.case_of(id), dtype, mutant))
    assert where in bad, (mutant, id, bad)


def test_mask_mutant_is_seen_in_the_backward_too():
    bad = dr.outside(run(dr.case_of("C-260"), torch.bfloat16, "mask_padded_pitch"))
    assert {"out32", "out16", "out_pe", "dx", "dy", "dgb"} <= set(bad), bad


@pytest.mark.parametrize("blocks", dr.REDUCE_BLOCKS)
def test_reduce_emulation_inside_its_bound_and_the_missing_tail_is_not(blocks):
    part, out0 = dr.reduce_inputs(blocks, 260, blocks)
    ref, bnd = dr.reduce_reference(part, out0), dr.reduce_bound(part, out0)
    rat = dr.ratios(dict(out=dr.reduce_emulate(part, out0)), dict(out=ref), dict(out=bnd))
    assert not dr.outside(rat) and rat["out"][0] <= 1.0 / dr.MARGIN, rat
    bad = dr.ratios(dict(out=dr.reduce_emulate(part, out0, "reduce_no_tail")), dict(out=ref), dict(out=bnd))
    if blocks % 16:                                     # 16 and 512 have no tail
        assert dr.outside(bad), (blocks, bad)
    else:
        assert not dr.outside(bad)
    assert blocks != 13 or bad["out"][1] > 260          # the named case: 13 blocks, one unrolled step + one tail row


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_flat_emulations_inside_their_bounds_and_the_relu_gate_mutant_is_not(dtype):
    n, p = 4096, 0.1
    h = dr.flat_inputs(n, dtype, 1)
    keep = dr.keep_mask(dr.SEED, dr.SALT, p, 1, n).reshape(n)
    ref = dr.relu_dropout_reference(h, keep, p)
    out = dr.relu_dropout_emulate(h, keep, p)
    rat = dr.ratios(dict(h=out), dict(h=ref), dict(h=dr.scaled_bound(ref, dtype)))
    assert not dr.outside(rat) and rat["h"][0] <= 1.0 / dr.MARGIN, rat
    assert bool((out.view(torch.int16)[ref == 0] == 0).all())                 # +0 exactly where dropped or h <= 0
    d = dr.flat_inputs(n, dtype, 2).roll(13)
    refb = dr.relu_dropout_bwd_reference(out, d, p)
    bnd = dict(d=dr.scaled_bound(refb, dtype))
    rat = dr.ratios(dict(d=dr.relu_dropout_bwd_emulate(out, d, p)), dict(d=refb), bnd)
    assert not dr.outside(rat) and rat["d"][0] <= 1.0 / dr.MARGIN, rat
    bad = dr.ratios(dict(d=dr.relu_dropout_bwd_emulate(out, d, p, "relu_gate_from_grad")), dict(d=refb), bnd)
    assert bad["d"][1] > n // 8, bad
    for count in dr.ADDN_COUNTS:
        for dt in (dtype, torch.float32):
            srcs = dr.addn_sources(count, 8 * 37, dt, count)
            tot, bnd = dr.sum_bound(srcs, None if dt is torch.float32 else dt)
            rat = dr.ratios(dict(s=dr.add_n_emulate(srcs, dt)), dict(s=tot), dict(s=bnd))
            assert not dr.outside(rat) and rat["s"][0] <= 1.0 / dr.MARGIN, (count, dt, rat)


def test_one_wrong_row_is_seen():
    """what a whole-tensor norm hides: the last of 2053 rows normalised with the neighbouring row's statistics"""
    c = dr.case_of("stride-bwd")
    inp, keep = dr.case_inputs(c, torch.bfloat16), dr.case_mask(c)
    got = dr.emulate(inp, keep, c["p"], torch.bfloat16)
    ref = dr.reference(inp, keep, c["p"])
    bnd = dr.bounds(ref, torch.bfloat16)
    R = c["R"]
    r = (ref["r"][R - 1] - ref["mu"][R - 2]) * ref["rstd_col"][R - 2]
    got["out32"] = got["out32"].clone()
    got["out32"][R - 1] = (r * ref["gamma"] + inp["beta"].double()).float()
    rel = float((got["out32"].double() - ref["out32"]).norm() / ref["out32"].norm())
    assert rel < 5e-3                                   # a norm test at the old suite's loosest threshold passes
    bad = dr.outside(dr.ln_ratios(got, ref, bnd))
    assert set(bad) == {"out32"} and bad["out32"][1] > c["C"] // 2, bad


def test_restated_mask():
    n = 100000
    for p in (0.1, 0.5, 0.9):
        keep = dr.keep_mask(dr.SEED, dr.SALT, p, 1, n)
        rate = float(keep.float().mean())
        assert abs(rate - (1 - p)) < 5.0 * math.sqrt(p * (1 - p) / n), (p, rate)
    a = dr.keep_mask(dr.SEED, dr.SALT, 0.5, 1, n)
    assert torch.equal(a, dr.keep_mask(dr.SEED, dr.SALT, 0.5, 1, n))
    for other in (dr.keep_mask(dr.SEED, dr.SALT + 1, 0.5, 1, n), dr.keep_mask(dr.SEED + 1, dr.SALT, 0.5, 1, n)):
        assert 0.49 < float((a == other).float().mean()) < 0.51
    assert torch.equal(dr.keep_mask(dr.SEED, dr.SALT, 0.5, 250, 400).reshape(-1), a.reshape(-1))   # index = row C + c
    assert not torch.equal(dr.keep_mask(dr.SEED, dr.SALT, 0.5, 250, 400, pitch=512).reshape(-1), a.reshape(-1))
    assert dr.threshold(1e-12) == 1 and dr.threshold(0.0) == 0 and dr.threshold(0.5) == 2 ** 31
    assert dr.threshold(0.1) == int(dr.as_f32(0.1) * 2 ** 32) and dr.threshold(0.9999999) == 2 ** 32 - 512
    assert bool(dr.keep_mask(dr.SEED, dr.SALT, 0.0, 1, n).all())
    assert int((~dr.keep_mask(dr.SEED, dr.SALT, 1e-12, 1, n)).sum()) == 0                         # hash == 0: one in 2^32
    # dec_seed / dec_hash against values worked out by hand from csrc/common.h with Python integers
    s = (0x1234567887654321 * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * 6) % 2 ** 64
    assert dr.dec_seed(dr.SEED, dr.SALT) == ((s >> 32) ^ s) % 2 ** 32
    assert dr.dec_seed(-1, 0) == dr.dec_seed(2 ** 64 - 1, 0)                                       # an int64 tensor's view
    x = (7 ^ 0xDEADBEEF) * 0x9E3779B1 % 2 ** 32
    x ^= x >> 15
    x = x * 0x85EBCA77 % 2 ** 32
    x ^= x >> 13
    x = x * 0xC2B2AE3D % 2 ** 32
    x ^= x >> 16
    import numpy as np
    assert int(dr.dec_hash(np.array([7], dtype=np.uint32), 0xDEADBEEF)[0]) == x
