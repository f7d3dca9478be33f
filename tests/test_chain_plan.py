"""models/chain_plan.py: where the prefetched sampling chain of Pointnet2Backbone puts the pieces of its flat buffer, and the
views that read them.  Host only: integers, and int32 tensors on the CPU."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

import chain_plan


def _cases():
    with open(os.path.join(GOLDEN, "chain_layout.json")) as fh:
        return json.load(fh)["cases"]


def _r4(n):
    return (n + 3) // 4 * 4


def _layout(B, n_points, plan_extra=None):
    """the layout a chain launched now gets, through the backbone (which asks sa_fused's switches)"""
    import backbone_module
    net = backbone_module.Pointnet2Backbone()
    net.plan_extra = plan_extra
    return net._chain_layout(B, n_points)


def _case_layout(case, monkeypatch):
    import sa_fused
    assert sa_fused.PLAN_MIN_ROWS == case["plan_min_rows"]
    monkeypatch.setattr(sa_fused, "ROW_PLAN", case["row_plan"])
    return _layout(case["B"], case["n_points"], case["plan_extra"])


def _as_recorded(layout):
    """a ChainLayout in the positional form the golden table was recorded in (make_golden_chain_layout.py)"""
    levels = [[s.name, s.M, s.S, s.n_src, s.xyz, s.idx, s.plan, s.csr_offsets, s.inds] for s in layout.stages]
    fps = [list(f) for f in layout.fps]
    return {"total": layout.total, "levels": levels, "fps": fps, "extra": None if layout.extra is None else list(layout.extra)}


def _pieces(layout, B, plan_words):
    """[(label, first word, words in use)] of every piece, from the documented shapes"""
    out = []
    for i, s in enumerate(layout.stages):
        P = B * s.M * s.S
        out += [(s.name + ".inds", s.inds, B * s.M), (s.name + ".xyz", s.xyz, B * s.M * 3), (s.name + ".idx", s.idx, P)]
        if s.plan is not None:
            out.append((s.name + ".plan", s.plan, plan_words[i]))
        if s.csr_offsets is not None:
            out += [(s.name + ".csr_offsets", s.csr_offsets, B * (s.n_src + 1)), (s.name + ".csr_order", s.csr_order, P)]
    for j, f in enumerate(layout.fps):
        out += [(f"fp{j}.weight", f.weight, B * f.n * 3), (f"fp{j}.idx", f.idx, B * f.n * 3),
                (f"fp{j}.csr_offsets", f.csr_offsets, B * (f.m + 1)), (f"fp{j}.csr_order", f.csr_order, B * f.n * 3)]
    if layout.extra is not None:
        out.append(("extra.inds", layout.extra.inds, B * layout.extra.n))
    return out


def _check_invariants(layout, B, planned, plan_words):
    pieces = _pieces(layout, B, plan_words)
    assert all(at % 4 == 0 for _, at, _ in pieces), pieces
    assert all(None not in (s.inds, s.xyz, s.idx) for s in layout.stages)
    ordered = sorted(pieces, key=lambda p: p[1])
    assert ordered[0][1] >= 0
    for (la, a, na), (lb, b, _) in zip(ordered, ordered[1:]):
        assert na > 0 and a + na <= b, (la, lb)                                     # pairwise disjoint
    assert layout.total == _r4(ordered[-1][1] + ordered[-1][2])                     # ... inside [0, total), which ends the last
    assert [s.csr_offsets is not None for s in layout.stages] == [False, True, True, True]
    assert [s.csr_order is not None for s in layout.stages] == [False, True, True, True]
    assert [s.plan is not None for s in layout.stages] == [bool(p) for p in planned]


def _planned_and_words(B, layout):
    import sa_fused
    return ([sa_fused.plan_static_ok(s.S, B * s.M * s.S) for s in layout.stages],
            [sum(sa_fused.plan_words(B, s.M, B * s.M * s.S)) for s in layout.stages])


def test_chain_layout_equals_the_recorded_group_layout(built_lib, monkeypatch):
    """Every offset and the total of the six recorded cases (tests/golden/chain_layout.json: what _group_layout returned on
    the commit before chain_plan.py), the CSR's second piece where _group_views put it, and the invariants of a layout."""
    cases = _cases()
    assert [(c["B"], c["n_points"], c["plan_extra"], c["row_plan"]) for c in cases] == [
        (8, 40000, None, True), (8, 40000, {"sa2": 256}, True), (4, 40000, None, True), (2, 8192, None, True),
        (1, 1024, None, True), (8, 40000, None, False)]
    import sa_fused
    for case in cases:
        layout = _case_layout(case, monkeypatch)
        got = _as_recorded(layout)
        for k in ("total", "levels", "fps", "extra"):
            assert got[k] == case[k], (case["name"], k)
        B = case["B"]
        for s in layout.stages[1:]:
            assert s.csr_order == s.csr_offsets + _r4(B * (s.n_src + 1)), (case["name"], s.name)
        assert layout.plan_group == sa_fused.PLAN_GROUP
        planned, words = _planned_and_words(B, layout)
        _check_invariants(layout, B, planned, words)
    by_name = {c["name"]: c for c in cases}
    plans = lambda name: [lv[6] is not None for lv in by_name[name]["levels"]]
    assert plans("bench") == [True, True, False, False] and plans("b4_sa2_at_min_rows") == [True, True, False, False]
    assert plans("b2_8192_sa1_only") == [True, False, False, False] and plans("bench_row_plan_off") == [False] * 4
    # (sa1 has 2048 x 64 = PLAN_MIN_ROWS grouped rows per scene whatever the cloud's size: one scene is planned already)
    assert plans("b1_1024") == [True, False, False, False]


def test_a_slot_with_two_fields_swapped_does_not_match_the_record(built_lib, monkeypatch):
    case = _cases()[0]
    layout = _case_layout(case, monkeypatch)
    assert _as_recorded(layout)["levels"] == case["levels"]
    s = layout.stages[1]
    swapped = layout._replace(stages=layout.stages[:1] + (s._replace(idx=s.xyz, xyz=s.idx),) + layout.stages[2:])
    assert _as_recorded(swapped)["levels"] != case["levels"]


def test_chain_layout_invariants_on_a_sweep(built_lib):
    for B in range(1, 10):
        for n in (256, 1000, 8192, 40000):
            for extra in (None, {"sa2": 256}):
                layout = _layout(B, n, extra)
                planned, words = _planned_and_words(B, layout)
                _check_invariants(layout, B, planned, words)
                assert (layout.extra is None) == (extra is None)
    # a plan slot follows `planned` alone, whatever the geometry says
    stages = (("sa1", 2048, 64), ("sa2", 1024, 32), ("sa3", 512, 16), ("sa4", 256, 16))
    for bits in range(16):
        planned = [bool(bits >> i & 1) for i in range(4)]
        words = [4 * (37 + i) for i in range(4)]
        layout = chain_plan.chain_layout(3, 1000, stages, planned, words, ((2, 3), (1, 2)), ("sa2", 77), 16)
        _check_invariants(layout, 3, planned, words)


@pytest.mark.parametrize("B,n,extra", [(2, 8192, {"sa2": 256}), (1, 1000, None), (8, 40000, {"sa2": 256})])
def test_chain_views_are_the_slots_words(built_lib, B, n, extra):
    """On an int32 arange buffer: every view has the documented shape and dtype, starts at its slot's offset and covers only
    its slot's words."""
    layout = _layout(B, n, extra)
    planned, words = _planned_and_words(B, layout)
    assert planned[0]
    base = torch.arange(layout.total, dtype=torch.int32)
    flat = base.clone()
    views = chain_plan.chain_views(flat, layout, B, planned)
    i32, f32 = torch.int32, torch.float32
    listed = []                     # (label, view, first word, shape, dtype)
    for i, (s, v) in enumerate(zip(layout.stages, views.stages)):
        listed += [(s.name + ".centres", v.centres, s.xyz, (B, s.M, 3), f32), (s.name + ".idx", v.idx, s.idx, (B, s.M, s.S), i32),
                   (s.name + ".inds", v.inds, s.inds, (B, s.M), i32)]
        assert (v.plan_state is None) == (s.plan is None) and (v.csr is None) == (s.csr_offsets is None)
        assert v.planned == (planned[i] and s.plan is not None)
        if s.plan is not None:
            listed.append((s.name + ".plan", v.plan_state, s.plan, (words[i],), i32))
        if s.csr_offsets is not None:
            listed += [(s.name + ".csr.offsets", v.csr.offsets, s.csr_offsets, (B, s.n_src + 1), i32),
                       (s.name + ".csr.order", v.csr.order, s.csr_order, (B, s.M * s.S), i32)]
            assert v.csr.space == ((v.plan_state.data_ptr(), layout.plan_group) if v.planned else None)
    for j, (f, v) in enumerate(zip(layout.fps, views.fps)):
        assert v.unknown is views.stages[f.unknown].centres and v.known is views.stages[f.known].centres
        assert v.csr.space is None
        listed += [(f"fp{j}.weight", v.weight, f.weight, (B, f.n, 3), f32), (f"fp{j}.idx", v.idx, f.idx, (B, f.n, 3), i32),
                   (f"fp{j}.csr.offsets", v.csr.offsets, f.csr_offsets, (B, f.m + 1), i32),
                   (f"fp{j}.csr.order", v.csr.order, f.csr_order, (B, f.n * 3), i32)]
    assert (views.extra is None) == (extra is None)
    if extra is not None:
        listed.append(("extra", views.extra, layout.extra.inds, (B, layout.extra.n), i32))
    assert len(listed) == len(_pieces(layout, B, words))
    for label, view, at, shape, dtype in listed:
        assert tuple(view.shape) == shape and view.dtype == dtype, label
        words_of = view.view(torch.int32).reshape(-1)
        assert int(words_of[0]) == at, label
        words_of.fill_(-1)                                              # the sentinel, through the view
        touched = (flat != base).nonzero().reshape(-1)
        assert touched.numel() == words_of.numel() and int(touched[0]) == at and int(touched[-1]) == at + words_of.numel() - 1, label
        words_of.copy_(base[at:at + words_of.numel()])
    assert torch.equal(flat, base)
    # without `planned` (a buffer about to be filled) no CSR names a plan's row space
    assert all(v.csr is None or v.csr.space is None for v in chain_plan.chain_views(flat, layout, B).stages)
