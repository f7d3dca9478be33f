"""CPU only: the host side of the prediction heads (models/pred_heads.py) issues exactly the C-ABI calls it issued while it was
part of models/pq_transformer.py.  tests/golden/heads_calls.json was RECORDED from that earlier commit by
tests/golden/make_golden_heads_calls.py, which also defines the cases and the recorder: the three decode nodes on their own
(with and without a sink, with the positions' 16-bit rows on and off), the pair / stacks / single routes, the grouped route
of 1, 3 and 7 stages (all reaching the loss, only the first and the last, a stage of another geometry, no sink), every switch
off -- each with dense gradients for every output and with one output unused.  Nothing is launched: `_call` is the recorder,
so the tensors live on the CPU."""
import importlib.util
import json
import os

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_heads_calls", os.path.join(GOLDEN, "make_golden_heads_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_heads_issue_the_recorded_calls(built_lib):
    gen = _generator()
    with open(os.path.join(GOLDEN, "heads_calls.json")) as fh:
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
