"""GPU: how many times the whole model calls each C entry point in one forward + backward (the fixture of
test_gpu_heads_bwd_group_model.py: batch 2, 8192 points, bf16, the same dropout seed; pointnet2/_ext.py: set_timing_sink), with
the defaults and with _HEADS_BWD_GROUP, _PAIR_DECODE and _PAIR_STACKS off one at a time, equals
tests/golden/heads_model_call_counts.json.  That table was recorded by `record()` below -- this test's own body -- on the commit
BEFORE the heads moved into models/pred_heads.py."""
import collections
import json
import os

import pytest
import torch

from conftest import GOLDEN
from test_gpu_heads_bwd_group_model import DEV, model  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
TABLE = os.path.join(GOLDEN, "heads_model_call_counts.json")
OFF = (None, "_HEADS_BWD_GROUP", "_PAIR_DECODE", "_PAIR_STACKS")


def counts(net, pc, module, off):
    """-> {entry point: calls} of one forward + backward with the switch `off` of `module` off (None: the defaults)"""
    import bench
    import dropout_state
    import sa_fused
    calls = []
    before = None if off is None else getattr(module, off)
    try:
        if off is not None:
            setattr(module, off, False)
        dropout_state.STATE.set_state(torch.device(DEV), 0x5EED5EED)
        net.zero_grad(set_to_none=True)
        sa_fused._ext.set_timing_sink(calls)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = bench.loss_of(net({"point_clouds": pc}))
        with sa_fused.deferred_wgrads():
            loss.backward()
        torch.cuda.synchronize()
    finally:
        sa_fused._ext.set_timing_sink(None)
        if off is not None:
            setattr(module, off, before)
    return dict(sorted(collections.Counter(c[0] for c in calls).items()))


def all_counts(net, pc, module):
    return {"defaults" if off is None else off: counts(net, pc, module, off) for off in OFF}


def record(path, module_name="pred_heads"):
    """Write the table (not a test; run by hand on the commit the table is to come from, where the switches lived in
    `module_name`): python -c "import sys; sys.path[:0] = ['tests']; import test_gpu_heads_call_counts as t; t.record(PATH, MOD)" """
    import importlib
    import bench
    import synth
    from procedural import load_procedural
    import test_gpu_heads_bwd_group_model as fixture
    pc = synth.make_clouds(90, 2, 8192, kind="room").to(DEV)
    net = load_procedural(bench.build_model(0)).to(DEV).train()
    fixture.run_once(net, pc, False)
    with open(path, "w") as fh:
        json.dump(all_counts(net, pc, importlib.import_module(module_name)), fh, indent=0, sort_keys=True)
        fh.write("\n")


def test_the_model_calls_every_entry_point_as_often_as_before(model):  # noqa: F811
    import pred_heads
    net, pc = model
    with open(TABLE) as fh:
        want = json.load(fh)
    got = all_counts(net, pc, pred_heads)
    assert sorted(got) == sorted(want)
    for case in want:
        diff = {n: (got[case].get(n, 0), want[case].get(n, 0)) for n in set(got[case]) | set(want[case])
                if got[case].get(n, 0) != want[case].get(n, 0)}
        assert diff == {}, (case, diff)
    assert want["defaults"]["omnipq_decode_pair_group_bwd"] >= 1 and "omnipq_decode_pair_bwd" not in want["defaults"]
