"""CPU only: pointnet2/rows_mlp.py issues, for every stack the model runs and for the edges of every route, exactly the C-ABI
calls it issued before its routes were put into `stack_route()`.  tests/golden/rows_mlp_calls.json was RECORDED from that
earlier commit by tests/golden/make_golden_rows_calls.py, which also defines the cases and the recorder (entry point, every
number, which pointers are null and which alias inside a call, every pair hold): lone stacks and pairs, with and without an
input gradient, training and eval, dropout on and off, inside deferred_wgrads, with the collectives forced, every switch off.
Nothing is launched: `_call` is the recorder, so the tensors live on the CPU."""
import importlib.util
import json
import os

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_rows_calls", os.path.join(GOLDEN, "make_golden_rows_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rows_mlp_issues_the_recorded_calls(built_lib):
    gen = _generator()
    with open(os.path.join(GOLDEN, "rows_mlp_calls.json")) as fh:
        table = json.load(fh)
    cases = gen.cases()
    # the table is the generator's list of cases, in its order (a case added there needs a new recording)
    assert [name for name, _ in table["cases"]] == [name for name, _ in cases]
    assert len(table["sequences"]) == len({tuple(s) for s in table["sequences"]})          # each distinct sequence once
    want = gen.expand(table)
    for name, case in cases:
        got = json.loads(json.dumps(gen.run_case(case)))
        assert len(got) == len(want[name]), (name, len(got), len(want[name]))
        wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want[name])) if g != w]
        assert wrong == [], (name, wrong[:3])
