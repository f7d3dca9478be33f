"""CPU: the float64 reference, the elementwise bound and the emulation of omnipq_sa_infer's arithmetic agree with each other
on every case both suites walk (tests/sa_infer_reference.py) -- the faithful emulation is inside the bound at every element of
both outputs, and each of the eight mutants is outside it at some element of every case it applies to.  No library, no GPU."""
import pytest
import torch

import sa_infer_reference as R


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_faithful_emulation_is_within_the_bound_everywhere(id):
    case = R.case_of(id)
    inp, ref = R.case_data(id)
    B, N, M, S = case["shape"]
    assert tuple(ref["out"].shape) == (B * M, case["widths"][-1])
    assert bool((ref["bound_f32"] > 0).all()) and bool(torch.isfinite(ref["bound_pm"]).all())
    # the case is not degenerate: most channels are alive, the dead ones (relu's zero in every row) are there
    alive = (ref["out"] > 0).double().mean()
    assert 0.5 < float(alive) < 1.0, float(alive)
    got_f32, got_pm = R.emulate(inp, case["shape"], case["cin"], case["dtype"])
    rat = R.ratios(got_f32, got_pm, ref)
    print(id, R.fmt(rat))
    assert not R.outside(rat), rat
    assert torch.equal(got_pm, got_f32.to(case["dtype"]))


@pytest.mark.parametrize("mutant", R.MUTANTS)
@pytest.mark.parametrize("id", R.CASE_IDS)
def test_every_mutant_is_outside_the_bound_somewhere(id, mutant):
    case = R.case_of(id)
    if not R.applies(mutant, case):
        return                                            # the defect cannot change this shape's result
    inp, ref = R.case_data(id)
    got_f32, got_pm = R.emulate(inp, case["shape"], case["cin"], case["dtype"], mutant=mutant)
    rat = R.ratios(got_f32, got_pm, ref)
    print(id, mutant, R.fmt(rat))
    assert rat["out_f32"][1] > 0 and rat["out_pm"][1] > 0, (mutant, rat)


def test_every_mutant_applies_somewhere_and_the_table_holds_what_it_promises():
    for mutant in R.MUTANTS:
        assert sum(R.applies(mutant, c) for c in R.CASES) >= 4, mutant
    names = {c["name"]: c for c in R.CASES}
    assert len(R.CASES) == 2 * len(names) == 18
    B, N, M, S = names["partial-tile"]["shape"]
    assert (B * M * S) % R.tile_rows(S) != 0
    assert R.kpad_of(names["kpad544"]["cin"]) == 544 and R.kpad_of(names["odd-widths-kpad320"]["cin"]) == 320
    assert R.tile_rows(names["one-ball-per-tile"]["shape"][3]) == 128
    # the ball-query case holds padded balls (copies of the ball's first neighbour)
    inp, _ = R.case_data("bf16-ball-query")
    idx = inp["idx"]
    assert bool(((idx[:, :, 1:] == idx[:, :, :1]).sum(dim=2) > 0).any())
    inp, _ = R.case_data("bf16-negative-gamma")
    assert all(bool((lay["gamma"] < 0).all()) for lay in inp["layers"])
    var = torch.cat([lay["var"][R.PROBES:] for lay in inp["layers"][:1]])
    assert float(var.min()) < 1e-2 and float(var.max()) > 1.0
