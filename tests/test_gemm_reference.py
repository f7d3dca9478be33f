"""CPU: the float64 GEMM reference and its elementwise bounds (tests/gemm_reference.py) have teeth, and its restatement of
the dispatcher agrees with the library.

On every case the GPU suite runs (tests/test_gpu_gemm_f64.py walks the same table), a torch-CPU emulation of the kernels'
arithmetic -- f32 accumulation per 32-wide K-step, slabs summed in f32, then the bias, then one rounding -- stays inside every
bound, and each of seven plausible kernel defects put into that emulation leaves the bounds on a case with K <= 320 in both
element types.  The route every case must take is restated in gemm_reference.plan() and compared here with what the
library's workspace functions report (host code only: no GPU)."""
import ctypes

import pytest
import torch

import gemm_reference as gr


def run(id, mutant=None):
    case = gr.case_of(id)
    A, B, bias, ref, bnd = gr.case_data(id)
    cs0 = torch.full((case["M"],), gr.COLSUM_START) if case["entry"] == "tn_colsum" else None
    got = gr.emulate(case, A, B, bias, cs0, mutant)
    return got, gr.ratios(got, ref, bnd)


def test_case_table_covers_what_it_says():
    ids = gr.CASE_IDS
    assert len(set(ids)) == len(ids)
    assert {c["route"] for c in gr.CASES} == set(gr.ROUTES)
    # every case in both element types
    for dt in (torch.bfloat16, torch.float16):
        other = torch.float16 if dt is torch.bfloat16 else torch.bfloat16
        mine = {c["id"].split("-", 1)[1] for c in gr.CASES if c["dtype"] is dt}
        assert mine == {c["id"].split("-", 1)[1] for c in gr.CASES if c["dtype"] is other}
    bf = [c for c in gr.CASES if c["dtype"] is torch.bfloat16]

    def shapes(route, entry, **kw):
        return {(c["M"], c["N"], c["K"]) for c in bf if c["route"] == route and c["entry"] == entry
                and all(c[k] == v for k, v in kw.items())}

    res = {(1, 8, 32), (72, 40, 32), (130, 72, 320)}
    assert shapes("nt64-kres", "e16") == res and shapes("nt64-kres", "bias") == res
    assert shapes("nt64-stream", "f32") == res | {(72, 12, 32)}
    assert shapes("nt64-stream", "e16") == {(130, 72, 352), (77, 16, 544)} == shapes("nt64-stream", "bias")
    for entry in ("e16", "bias", "f32", "stats"):
        assert {(16400, 136, 96), (33000, 8, 32)} <= shapes("nt128", entry)
    assert (33000, 12, 32) in shapes("nt128", "f32")
    for bias in (False, True):
        assert shapes("ws-split64", "ws", bias=bias) >= {(72, 40, 800), (300, 96, 2048)}
        assert shapes("nt64-stream", "ws", bias=bias, ldc=48) == {(72, 40, 800)}
    assert {(c["M"], c["N"], c["K"], c["slabs"]) for c in bf if c["entry"] == "splitk"} == \
        {(72, 44, 96, 1), (72, 44, 96, 2), (72, 44, 96, 5), (200, 136, 96, 3)}
    tn = {(31, 8, 8), (32, 128, 128), (193, 72, 40), (6401, 8, 8), (1000, 136, 264)}        # (P, M, N)
    for entry in gr.TN_ENTRIES:
        assert {(c["K"], c["M"], c["N"]) for c in bf if c["entry"] == entry} == tn
    # the exact integer kind on the long and the ragged contractions of the f32 outputs
    assert {(c["entry"], c["M"], c["N"], c["K"]) for c in bf if c["kind"] == "int"} == {
        ("f32", 33000, 12, 32), ("splitk", 72, 44, 96), ("splitk", 200, 136, 96), ("tn_colsum", 8, 8, 31),
        ("tn_colsum", 72, 40, 193), ("tn_colsum", 8, 8, 6401), ("tn_colsum", 136, 264, 1000)}
    # padded pitches and the exact kind: once per route at least
    for route in gr.ROUTES:
        padded = [c for c in bf if c["route"] == route and c["lda"] > (c["M"] if route == "tn" else c["K"])]
        assert padded and any(c["kind"] == "onehot" for c in padded), route
        for c in padded:
            if route == "tn":
                assert (c["lda"], c["ldb"], c["ldc"]) == (c["M"] + 8, c["N"] + 16, c["N"])
            else:
                split = route in ("ws-split64", "splitk")
                assert (c["lda"], c["ldb"]) == (c["K"] + 8, c["K"] + 24)
                assert c["ldc"] == c["N"] + (0 if split else 4 if c["entry"] == "f32" else 8)
    # what the shapes are there for
    assert gr.plan(gr.case_of("bf16-ws-72x40x800"))["k_chunk"] == 288 and gr.plan(gr.case_of("bf16-ws-72x40x800"))["used"] == 3
    assert gr.plan(gr.case_of("bf16-ws-300x96x2048"))["used"] == 8
    assert [gr.plan(gr.case_of(f"bf16-splitk-s{s}-72x44x96"))["used"] for s in (1, 2, 5)] == [1, 2, 3]
    assert gr.plan(gr.case_of("bf16-tn-72x40x193"))["used"] == 2 and gr.plan(gr.case_of("bf16-tn-72x40x193"))["k_chunk"] == 128
    assert gr.plan(gr.case_of("bf16-tn-8x8x6401"))["used"] == 34 and gr.plan(gr.case_of("bf16-tn-8x8x6401"))["two_stage"]
    assert not any(gr.plan(c)["two_stage"] for c in bf if c["K"] != 6401)
    assert all(gr.plan(c)["stats_partial"] for c in bf if c["entry"] == "stats")
    assert all(gr.cdiv(c["M"], 128) * gr.cdiv(c["N"], 128) == 258 for c in bf if c["route"] == "nt128")


@pytest.mark.parametrize("id", gr.CASE_IDS)
def test_route_restatement_agrees_with_the_library(id, built_lib):
    case = gr.case_of(id)
    p = gr.plan(case)
    assert p["route"] == case["route"]
    lib = ctypes.CDLL(built_lib if case["dtype"] is torch.bfloat16 else built_lib[:-3] + "_f16.so")
    for fn in ("omnipq_gemm_nt_workspace_floats", "omnipq_gemm_nt_stats_workspace_floats", "omnipq_gemm_tn_workspace_floats"):
        getattr(lib, fn).restype = ctypes.c_longlong
    M, N, K = case["M"], case["N"], case["K"]
    if case["entry"] in gr.TN_ENTRIES:
        tiles = gr.cdiv(M, 128) * gr.cdiv(N, 128)
        slabs = int(lib.omnipq_gemm_tn_slabs(tiles, ctypes.c_longlong(K), gr.GBK))
        assert slabs == gr.tn_slabs(M, N, K)
        assert int(lib.omnipq_gemm_tn_workspace_floats(M, N, K)) == p["ws_floats"] == (slabs + 16) * M * N
        assert p["used"] <= slabs and (p["used"] - 1) * p["k_chunk"] < K <= p["used"] * p["k_chunk"]
    elif case["entry"] == "splitk":
        assert p["ws_floats"] == case["slabs"] * M * N and p["used"] <= case["slabs"]
    else:
        ws = int(lib.omnipq_gemm_nt_workspace_floats(M, N, K))
        slabs = gr.ws_split_slabs(M, N, K)
        assert ws == (slabs * M * N if slabs > 1 else 0)
        if case["entry"] == "ws":
            assert ws == p["ws_floats"]
            assert (p["route"] == "ws-split64") == (ws > 0 and case["ldc"] == N)
        else:
            assert ws == 0                               # no case of another entry point has a shape that would split
        stats_ws = int(lib.omnipq_gemm_nt_stats_workspace_floats(M, N))
        assert stats_ws == (gr.cdiv(M, 128) * 2 * N if gr.stats_partial(M) else 0)
        if case["entry"] == "stats":
            assert stats_ws == p["stats_ws_floats"] > 0


@pytest.mark.parametrize("id", gr.CASE_IDS)
def test_emulated_kernel_arithmetic_is_inside_every_bound(id):
    case = gr.case_of(id)
    got, rat = run(id)
    assert set(rat) == ({"C", "colsum"} if case["entry"] == "tn_colsum" else {"C"})
    assert not gr.outside(rat), (id, gr.fmt(rat))
    # the margin of 1.5 is for what the emulation does not do (the MFMA's summation order): it must not need it
    assert max(r[0] for r in rat.values()) <= 1.0 / gr.MARGIN, (id, gr.fmt(rat))
    if case["kind"] in gr.EXACT_KINDS:
        A, B, bias, ref, bnd = gr.case_data(id)
        assert all(torch.equal(got[n].double(), ref[n]) for n in got)
    if case["kind"] == "onehot":
        want = gr.onehot_expected(case, B)
        assert torch.equal(ref["C"], want.double())
        if gr.out_f32(case):
            assert torch.equal(got["C"], want.float())
        else:
            assert torch.equal(got["C"].view(torch.int16), want.view(torch.int16))


# (mutant, case without its library prefix): every one at K <= 320, in both element types
MUTANT_CASES = [
    ("drop_last_kstep", "bias-130x72x320-pad"),         # the last K-step dropped
    ("bias_after_round", "bias-130x72x320-pad"),        # bias added after the rounding: two roundings
    ("round_partials", "splitk-s3-200x136x96"),         # split-K partials rounded to e16 before they are summed
    ("truncate", "bias-130x72x320-pad"),                # truncation instead of round-to-nearest on store
    ("leak_row", "bias-130x72x320-pad"),                # a row past M leaks into the last stored row, scaled by 2^-7
    ("pitch_k", "bias-130x72x320-pad"),                 # K used as the pitch of A when lda > K
    ("swap_pieces", "bias-130x72x320-pad"),             # two 8-wide column pieces of the stored tile swapped
]


@pytest.mark.parametrize("lib", ["bf16", "f16"])
@pytest.mark.parametrize("mutant,name", MUTANT_CASES)
def test_mutant_leaves_a_bound(mutant, name, lib):
    assert {m for m, _ in MUTANT_CASES} == set(gr.MUTANTS)
    id = f"{lib}-{name}"
    assert gr.case_of(id)["K"] <= 320
    assert not gr.outside(run(id)[1])
    rat = run(id, mutant)[1]
    print(f"\n  MUTANT {mutant} {id}: {gr.fmt(rat)} outside={rat['C'][1]}")
    assert "C" in gr.outside(rat), (mutant, id, rat)


def test_one_wrong_element_is_seen():
    """what a whole-matrix tolerance hides: one element of size ~0.5 off by 3 % while the matrix maximum is several units"""
    id = "bf16-e16-16400x136x96"
    A, B, bias, ref, bnd = gr.case_data(id)
    got = gr.emulate(gr.case_of(id), A, B, bias)
    c = got["C"].float()
    want = ref["C"]
    at = int(((want.abs() - 0.5).abs()).flatten().argmin())
    err = 8 * 2.0 ** -8 * float(want.flatten()[at].abs())
    assert err < 2.0 ** -8 * float(want.abs().max())    # the old global tolerance lets it through
    c.view(-1)[at] += err
    bad = gr.outside(gr.ratios(dict(C=c), ref, bnd))
    assert {n: r[1] for n, r in bad.items()} == {"C": 1}, bad


def test_nonfinite_and_zero_bound_elements_count_as_outside():
    ref, bnd = dict(C=torch.zeros(2, 3, dtype=torch.float64)), dict(C=torch.zeros(2, 3, dtype=torch.float64))
    got = torch.zeros(2, 3)
    assert gr.ratios(dict(C=got), ref, bnd)["C"] == (0.0, 0)
    got[0, 1] = float("nan")
    got[1, 2] = 1e-30
    r = gr.ratios(dict(C=got), ref, bnd)["C"]
    assert r[0] == float("inf") and r[1] == 2
