"""CPU: the float64 restatement of the layout F1 (tests/layout_f1_restatement.py) is the rule the kernel must reproduce -- it
gives the reference's own F1 on both golden cases, the host QUADAPCalculator's counts on seeded scenes around the threshold, the
hand-computed ceiling and floor lists of every merge case, and each of its mutants changes the counts of an input built for it.

Guards on the inputs (assertions, never skips): no compared distance lies within 1e-6 of the threshold, so neither the host's
float32 `same_point` nor a last-bit difference of a square root can decide a case."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import layout_f1_restatement as R
import loss_inputs
import test_parse_quads as TQ

GUARD = 1e-6
FAMILIES = {"walls": dict(seed=11, b=6, k=9, g=7, cols=3), "two_quads": dict(seed=23, b=8, k=4, g=5, cols=1)}


def golden_arrays(name):
    """the arrays of a golden case, built as tests/test_parse_quads.py::oracle_parse builds its lists"""
    from oracle import ap_oracle
    ep = TQ.case_inputs(name)
    _, _, corners, _, gt_corners = TQ.oracle_parse(ep, loss_inputs.EVAL_CONFIG)
    B = len(corners)
    k = max(max(len(c) for c in corners), 1)
    verts = np.zeros((B, k, 4, 3), np.float32)
    for i, lst in enumerate(corners):
        for j, q in enumerate(lst):
            verts[i, j] = q
    gverts = ap_oracle.decode_quads(ep["gt_quad_centers"], ep["gt_normal_vectors"], ep["gt_quad_sizes"])[2]
    sc = dict(count_f1=np.array([len(c) for c in corners], np.int32), verts4=verts, gt_verts4=gverts.astype(np.float32),
              num_total=ep["num_total_quads"], num_gt=ep["num_gt_quads"], horizontal=ep["horizontal_quads"])
    assert [len(x) for x in gt_corners] == [int(n) for n in R.layout_f1_scene(sc)[:, 2]]
    return sc


def host_counts(sc, calculated):
    """the host calculator's F1 on the list form of a scene dict"""
    import ap_helper_pq
    calc = ap_helper_pq.QUADAPCalculator(0.25, {1: "quad"})
    pred, gt, hz = R.to_lists(sc["count_f1"], sc["verts4"], sc["gt_verts4"], sc["num_total"], sc["horizontal"])
    empty = [[] for _ in pred]
    calc.step(empty, empty, pred, gt, [torch.from_numpy(x) for x in hz])
    return calc.compute_F1(calculated=calculated)


def guarded(seen, thr=R.SAME_THRES):
    d = np.asarray(seen, np.float64)
    return float(np.abs(d[np.isfinite(d)] - thr).min()) if d.size else np.inf


@pytest.mark.parametrize("name", TQ.CASES)
def test_restatement_reproduces_the_reference_f1_of_the_golden_cases(name):
    sc = golden_arrays(name)
    seen = []
    rows = R.layout_f1_scene(sc, seen=seen)
    plain, calc = float(TQ.GOLD[f"{name}.f1_plain"][0]), float(TQ.GOLD[f"{name}.f1_calculated"][0])
    assert R.f1_of(rows.sum(0), False) == pytest.approx(plain, abs=1e-12)
    assert R.f1_of(rows.sum(0), True) == pytest.approx(calc, abs=1e-12)
    assert (sc["count_f1"] == 2).any() and plain != calc and rows[:, 3].sum() > 0          # a two-quad scene that counts
    print(f"{name}: rows {rows.tolist()}, nearest distance to the threshold {guarded(seen):.6f}")
    assert guarded(seen) >= 0.013                    # measured on the CPU: 0.013 at the nearest; the cases decide nothing there


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_restatement_equals_the_host_calculator_on_scenes_around_the_threshold(family):
    kw = FAMILIES[family]
    sc = R.random_scenes(family=family, **kw)
    seen = []
    rows = R.layout_f1_scene(sc, seen=seen)
    # the generator delivers what the comparison needs
    assert guarded(seen) > GUARD, guarded(seen)
    assert ((rows[:, 0] > 0) & (rows[:, 1] > 0)).any(), rows.tolist()
    only_swapped = 0
    for s in range(kw["b"]):
        gt = R.to_lists(sc["count_f1"], sc["verts4"], sc["gt_verts4"], sc["num_total"], sc["horizontal"])[1][s]
        for j in range(int(sc["count_f1"][s])):
            same, swapped = R.match_orders(sc["verts4"][s, j], np.asarray(gt, np.float32).reshape(-1, 4, 3))
            only_swapped += swapped and not same
    assert only_swapped > 0
    if family == "two_quads":
        assert 0 < rows[:, 3].sum() < 2 * kw["b"], rows.tolist()       # some ceilings / floors count, some do not
    total = rows.sum(0)
    assert total[2] > 0
    for calculated in (False, True):
        assert host_counts(sc, calculated) == R.f1_of(total, calculated)                   # equal counts: bit-equal F1
    # the counts themselves, not only their quotient: scene by scene
    for s in range(kw["b"]):
        one = {k: v[s:s + 1] for k, v in sc.items()}
        if rows[s, 2] > 0:
            assert host_counts(one, True) == R.f1_of(rows[s], True), s


@pytest.mark.parametrize("passes", [True, False])
def test_exactly_representable_distances_at_the_threshold(passes):
    sc = R.boundary_scene(passes)
    seen = []
    rows = R.layout_f1_scene(sc, seen=seen)
    x = float(np.nextafter(np.float32(0.4), np.float32(0))) if passes else float(np.float32(0.4))
    assert set(seen) == {x}                          # sqrt(x x) == x: the distance IS the f32 offset
    assert rows.tolist() == [[1, 0, 1, 0]] if passes else rows.tolist() == [[0, 1, 1, 0]]
    assert host_counts(sc, False) == (1.0 if passes else 0.0)


@pytest.mark.parametrize("name", sorted(R.MERGE_CASES))
def test_ceiling_and_floor_lists_of_the_merge_cases(name):
    import ap_helper_pq
    q0, q1, want = R.MERGE_CASES[name]
    seen = []
    ceiling, floor = R.ceiling_and_floor(np.stack([q0, q1]), seen=seen)
    assert guarded(seen) > GUARD
    assert np.array_equal(np.stack(ceiling), np.array([(x, y, 2.5) for x, y in want], np.float32))
    assert np.array_equal(np.stack(floor), np.array([(x, y, 0.0) for x, y in want], np.float32))
    hc, hf = ap_helper_pq.QUADAPCalculator().get_ceiling_and_floor([q0, q1])
    assert np.array_equal(np.stack(hc), np.stack(ceiling)) and np.array_equal(np.stack(hf), np.stack(floor))
    assert all(np.asarray(e).dtype == np.float32 for e in hc + hf)
    merged = sum(not any(np.array_equal(e, c) for c in np.concatenate([q0, q1])) for e in ceiling)
    assert merged == {"no_merge": 0, "shared_corner": 1, "narrow_quad": 1, "two_in_reach": 1, "midpoint_only": 2}[name]
    # within reach of the expected lists both count; out of reach neither does
    for shift, tp_h in ((0.125, 2), (0.5, 0)):
        sc = R.merge_scene(name, shift)
        seen = []
        rows = R.layout_f1_scene(sc, seen=seen)
        assert guarded(seen) > GUARD
        assert rows[0, 3] == tp_h and rows[0, 0] == 1 and rows[0, 1] == 1 and rows[0, 2] == 1
        assert host_counts(sc, True) == R.f1_of(rows[0], True)


def test_ceiling_and_floor_are_scored_for_two_quads_only():
    """get_ceiling_and_floor appends one entry per visited corner in both branches: 2 n entries for n quads"""
    import ap_helper_pq
    rs = np.random.RandomState(3)
    for n in range(0, 6):
        quads = [R.wall(rs, width=0.2 + 0.3 * (j % 2)) for j in range(n)]
        hc, hf = ap_helper_pq.QUADAPCalculator().get_ceiling_and_floor(quads)
        assert len(hc) == len(hf) == 2 * n
        got = R.ceiling_and_floor(np.asarray(quads, np.float32).reshape(-1, 4, 3))
        assert [len(x) for x in got] == [2 * n, 2 * n]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_fails_on_the_input_built_for_it(mutant):
    sc = R.mutant_input(mutant)
    thr = sc.get("same_thres", R.SAME_THRES)
    seen = []
    rule = R.layout_f1_scene(sc, seen=seen)
    if mutant != "strict":                           # that input sits ON its threshold on purpose (exactly: 0.5)
        assert guarded(seen, thr) > GUARD
    else:
        assert 0.5 in seen
    wrong = R.layout_f1_scene(sc, mutant=mutant)
    assert not np.array_equal(rule, wrong), (rule.tolist(), wrong.tolist())
    if thr == R.SAME_THRES and rule[0, 2] > 0:       # and the host calculator sides with the rule
        for calculated in (False, True):
            assert host_counts(sc, calculated) == R.f1_of(rule[0], calculated)
            if R.f1_of(rule[0], calculated) != R.f1_of(wrong[0], calculated):
                assert host_counts(sc, calculated) != R.f1_of(wrong[0], calculated)
