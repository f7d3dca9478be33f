"""CPU only: pointnet2/sa_fused.py issues, for one set-abstraction stage on every value of every `StageRoute` field, exactly
the C-ABI calls it issued before its hidden arguments were made explicit.  tests/golden/sa_stage_calls.json was RECORDED from
that earlier commit by tests/golden/make_golden_sa_calls.py, which also defines the cases and the recorder.  The recorder
replaces `_ext._run`, one level below `sa_fused._call`, so per call it keeps the entry point, every number, which pointers are
null and which alias, the row plan the call was given (its rows, its group size, whether `pool_gamma` is set) and the timing
tag (the stage's label, forward and backward); per case the all-reduces of a world of two and the `*_uses` counters.
Nothing is launched: the tensors live on the CPU."""
import importlib.util
import json
import os

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_sa_calls", os.path.join(GOLDEN, "make_golden_sa_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sa_stage_issues_the_recorded_calls(built_lib):
    gen = _generator()
    with open(os.path.join(GOLDEN, "sa_stage_calls.json")) as fh:
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
