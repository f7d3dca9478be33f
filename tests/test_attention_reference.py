"""CPU: the float64 attention reference and its elementwise bounds (tests/attention_reference.py) have teeth.

On every case the GPU suite runs (tests/test_gpu_attention_f64.py walks the same table), a torch-CPU emulation of the
kernels' arithmetic -- f32, P rounded to e16 per key block under an online softmax, O rounded on store, delta from the
stored O, dS rounded to e16 -- stays inside every bound, and each of seven plausible kernel defects put into that emulation
leaves at least one bound on the case named for it.  No GPU: the keep masks here are Bernoulli draws, on the GPU they are
the kernels' own."""
import pytest
import torch

import attention_reference as ar


def run(case, mutant=None):
    q, k, v, do = ar.case_inputs(case)
    B, L, S, p = case["N"] * case["H"], case["L"], case["S"], case["p"]
    seed = ar.CASE_IDS.index(case["id"])
    mask = ar.bernoulli_mask(B, L, S, p, seed) if p > 0 else None
    other = ar.bernoulli_mask(B, L, S, p, seed + 1) if mutant == "bwd_other_mask" else None
    got = ar.emulate(q, k, v, do, mask, p, mutant, other)
    ref = ar.reference(q, k, v, do, mask, p)
    bnd = ar.bounds(ref, case["dtype"], o_stored=got["O"])
    return ar.ratios(got, ref, bnd, o_stored=got["O"])


def case(id):
    return ar.CASES[ar.CASE_IDS.index(id)]


def test_case_table_covers_what_it_says():
    ids = ar.CASE_IDS
    assert len(set(ids)) == len(ids)
    shapes = {(c["L"], c["S"]) for c in ar.CASES if c["id"].startswith("shape-")}
    assert shapes == {(L, S) for L in (1, 31, 32, 33, 65) for S in (1, 31, 33, 45, 128, 129, 160, 257)}
    assert sorted(c["D"] for c in ar.CASES if c["id"].startswith("headdim-")) == list(range(4, 49, 4))
    assert {c["layout"] for c in ar.CASES} == {"contig", "pitch4", "self", "cross", "own"}
    assert {c["N"] * c["H"] for c in ar.CASES if c["id"].startswith("xcd-")} == {6, 8, 16}
    assert {c["kind"] for c in ar.CASES} == {"randn", "big", "inc", "dec", "last", "equal", "neg80"}
    assert all(c["L"] == c["S"] for c in ar.CASES if c["layout"] == "self")
    assert all(c["D"] % 4 == 0 and c["D"] <= 48 for c in ar.CASES)


def test_inputs_are_what_their_kind_promises():
    q, k, v, do = ar.case_inputs(case("logits-inc"))
    s2 = ar.reference(q, k, v, do)
    s = s2["c"] * s2["q"] @ s2["k"].transpose(1, 2)
    blockmax = torch.stack([s[:, :, b:b + 32].max(dim=2).values for b in range(0, 129, 32)])
    assert bool((blockmax[1:] > blockmax[:-1]).all()) and bool((blockmax[3] > blockmax[0] + 20.0).all())              # every block raises every query's maximum
    q, k, v, do = ar.case_inputs(case("logits-dec"))
    s2 = ar.reference(q, k, v, do)
    s = s2["c"] * s2["q"] @ s2["k"].transpose(1, 2)
    blockmax = torch.stack([s[:, :, b:b + 32].max(dim=2).values for b in range(0, 129, 32)])
    assert bool((blockmax[1:] < blockmax[:-1]).all())
    for id, S in (("logits-last-45", 45), ("logits-last-129", 129)):
        r = ar.reference(*ar.case_inputs(case(id)))
        assert bool((r["P"][:, :, S - 1] > 0.99).all())
    r = ar.reference(*ar.case_inputs(case("logits-equal")))
    assert float((r["P"] - 1.0 / 129).abs().max()) < 1e-12
    s = (r["c"] * r["q"] @ r["k"].transpose(1, 2))[:, :, 0]
    assert float((r["lse2"] - (s * ar.LOG2E + torch.log2(torch.tensor(129.0, dtype=torch.float64)))).abs().max()) < 1e-9
    r = ar.reference(*ar.case_inputs(case("logits-neg80")))
    s = r["c"] * r["q"][0] @ r["k"][0].T
    assert -110.0 < float(s.min()) and float(s.max()) < -55.0
    r = ar.reference(*ar.case_inputs(case("logits-big")))
    s = r["c"] * r["q"] @ r["k"].transpose(1, 2)
    assert float(s.max()) > 60.0


def test_reference_agrees_with_autograd():
    """the closed-form backward of the reference is the derivative of its forward"""
    c = case("dropout-0.5-33x130")
    q, k, v, do = (t.double().requires_grad_(True) for t in ar.case_inputs(c))
    mask = ar.bernoulli_mask(4, 33, 130, 0.5, 3)
    w = torch.softmax(q @ k.transpose(1, 2) * 36 ** -0.5, dim=2) * mask.double() / 0.5
    o = w @ v
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], do.detach())
    r = ar.reference(q.detach(), k.detach(), v.detach(), do.detach(), mask, 0.5)
    for a, b in ((o, r["O"]), (dq, r["dQ"]), (dk, r["dK"]), (dv, r["dV"])):
        assert float((a.detach() - b).abs().max()) <= 1e-12 * float(b.abs().max())
    lse = torch.logsumexp(q.detach() @ k.detach().transpose(1, 2) * 36 ** -0.5, dim=2) * ar.LOG2E
    assert float((lse - r["lse2"]).abs().max()) < 1e-10


@pytest.mark.parametrize("id", ar.CASE_IDS)
def test_emulated_kernel_arithmetic_is_inside_every_bound(id):
    rat = run(case(id))
    assert set(rat) == set(ar.OUTPUTS)
    assert not ar.outside(rat), (id, ar.fmt(rat))
    # the margin of 1.5 is for what the emulation does not do (MFMA summation order, hardware exp2): it must not need it
    assert max(rat[n][0] for n in ("O", "dQ", "dK", "dV")) <= 1.0 / ar.MARGIN, (id, ar.fmt(rat))


MUTANT_CASES = [
    ("drop_last_key", "shape-33x45", "O"),              # the last key of a partial block ignored
    ("ln_lse", "shape-33x45", "lse2"),                  # natural log instead of log2
    ("delta_no_mask", "dropout-0.5-33x130", "dQ"),      # delta without the dropout mask
    ("bwd_other_mask", "dropout-0.1-33x130", "dV"),     # backward draws the mask of another salt
    ("dk_no_scale", "shape-33x45", "dK"),               # dK without the factor c
    ("half_swap", "shape-33x45", "O"),                  # keys 4h..4h+3 of each 8 exchanged between the lane halves
    ("no_rescale", "logits-inc", "O"),                  # running output not rescaled when a later block raises the maximum
]


@pytest.mark.parametrize("mutant,id,where", MUTANT_CASES)
def test_mutant_leaves_a_bound(mutant, id, where):
    assert {m for m, _, _ in MUTANT_CASES} == set(ar.MUTANTS)
    assert not ar.outside(run(case(id)))
    bad = ar.outside(run(case(id), mutant))
    assert where in bad, (mutant, id, bad)


def test_one_wrong_element_is_seen():
    """what a whole-tensor norm hides: one element of dK off by 3 %, one lse2 off by 1e-3"""
    c = case("shape-33x257")
    q, k, v, do = ar.case_inputs(c)
    got = ar.emulate(q, k, v, do)
    ref = ar.reference(q, k, v, do)
    bnd = ar.bounds(ref, c["dtype"], o_stored=got["O"])
    dk = got["dK"].float()
    rel = (8 * 2.0 ** -8 * ref["dK"].abs() / bnd["dK"]).flatten()
    at = int(rel.argmax())                              # an element whose own size dominates its bound
    assert float(rel[at]) > 2.0
    dk.view(-1)[at] *= 1.0 + 8 * 2.0 ** -8
    got["dK"] = dk
    got["lse2"] = got["lse2"].clone()
    got["lse2"][0, 5] += 1e-3
    bad = ar.outside(ar.ratios(got, ref, bnd, o_stored=got["O"]))
    assert {n: r[1] for n, r in bad.items()} == {"dK": 1, "lse2": 1}, bad
