"""CPU: the float64 reference, the elementwise bound and the emulation of omnipq_rows_infer's arithmetic agree with each other
on every case both suites walk (tests/rows_infer_reference.py) -- the faithful emulation is inside the bound at every element,
and each mutant is outside it at some element of every case it applies to.  No library, no GPU."""
import pytest
import torch

import rows_infer_reference as R


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_faithful_emulation_is_within_the_bound_everywhere(id):
    case = R.case_of(id)
    inp, ref = R.case_data(id)
    n, widths = R.rows_of(case), R.widths_of(case)
    C = case["layers"][-1][0]
    assert tuple(ref["out"].shape) == (n, widths[-1])
    assert bool((ref["bound"][:, :C] > 0).all()) and bool(torch.isfinite(ref["bound"]).all())
    # padded columns: exact zeros, and nothing in the bound but every layer's eta (the suites assert exact zeros themselves)
    assert bool((ref["out"][:, C:] == 0).all()) and bool((ref["bound"][:, C:] == R.abs_roundoff(case["dtype"])).all())
    # the case is not degenerate
    alive = (ref["out"][:, :C] != 0).double().mean()
    assert float(alive) > 0.4, float(alive)
    got = R.emulate(inp, case["cin"], case["dtype"])
    rat = R.ratios(got, ref)
    print(id, R.fmt(rat))
    assert not R.outside(rat), rat
    assert bool((got[:, C:] == 0).all())


@pytest.mark.parametrize("mutant", [m for m in R.MUTANTS if m not in R.INVISIBLE])
@pytest.mark.parametrize("id", R.CASE_IDS)
def test_every_mutant_is_outside_the_bound_somewhere(id, mutant):
    case = R.case_of(id)
    if not R.applies(mutant, case):
        return                                            # the defect cannot change this shape's result
    inp, ref = R.case_data(id)
    rat = R.ratios(R.emulate(inp, case["cin"], case["dtype"], mutant=mutant), ref)
    print(id, mutant, R.fmt(rat))
    assert rat["out"][1] > 0, (mutant, rat)


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_rows_do_not_meet_so_a_partial_tiles_missing_rows_cannot_show(id):
    """the one mutant a bound cannot see (R.INVISIBLE): whatever the rows behind n hold, the n output rows are the same bits"""
    case = R.case_of(id)
    inp, _ = R.case_data(id)
    want = R.emulate(inp, case["cin"], case["dtype"])
    got = R.emulate(inp, case["cin"], case["dtype"], mutant="partial_tile_row0")
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_every_mutant_applies_somewhere_and_the_table_holds_what_it_promises():
    for mutant in R.MUTANTS:
        if mutant in R.INVISIBLE:
            assert not any(R.applies(mutant, c) for c in R.CASES)
        else:
            assert sum(R.applies(mutant, c) for c in R.CASES) >= 4, mutant
    names = {c["name"]: c for c in R.CASES}
    assert len(R.CASES) == 2 * len(names) == 24
    assert names["pos-pitch6"]["ldx"] == 6 and names["pos"]["ldx"] == 3 and names["pos"]["x_dtype"] == torch.float32
    assert R.rows_of(names["one-row"]) == 1 and R.rows_of(names["persistent"]) == 64 * 2 * R.ASSUMED_CUS + 5
    # partial tiles, whole tiles, and the one shape that needs the 32-row tile
    assert R.rows_of(names["pos"]) % 64 and R.rows_of(names["pos6"]) % 64 == 0
    assert R.lds_bytes(1024, (512, 512)) == (8 * 1024 + 2 * 32 * (1032 + 520), 32)
    assert all(R.lds_bytes(R.kpad_of(c), R.widths_of(c))[1] == 64 for c in R.CASES if c["name"] != "1024-512-512")
    assert R.widths_of(names["vote"]) == (288, 288, 320) and R.widths_of(names["head"]) == (288, 288, 128)
    inp, _ = R.case_data("bf16-negative-gamma")
    assert all(bool((lay["gamma"] < 0).all()) for lay in inp["layers"] if lay["gamma"] is not None)
    var = inp["layers"][0]["var"][R.PROBES:]
    assert float(var.min()) < 1e-2 and float(var.max()) > 1.0
    inp, _ = R.case_data("bf16-vote")
    assert all(float(lay["bias"].abs().max()) > 0.1 for lay in inp["layers"])          # conv biases non-zero
    inp, _ = R.case_data("bf16-fp")
    assert all(lay["bias"] is None for lay in inp["layers"]) and inp["layers"][-1]["relu"]
    inp, _ = R.case_data("bf16-pos-pitch6")
    assert bool((inp["x"][:, 3:] == R.JUNK).all())
