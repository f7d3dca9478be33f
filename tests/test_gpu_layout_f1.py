"""GPU: the layout F1 on the device (csrc/layout_f1.hip; ap_helper_pq.LayoutF1, QUADAPCalculator(f1="device");
inference.evaluate_layout_f1) against the float64 restatement (tests/layout_f1_restatement.py), the reference's golden F1 and
the host calculator.

The outputs are integer counts and are compared EXACTLY.  What makes that sound is a guard on every input, asserted on the CPU
before the comparison: no distance the rule compares lies within 1e-6 of the threshold (the restatement collects them all), so
the last bit of a square root cannot decide a case; the two inputs that sit on a threshold on purpose do so with exactly
representable distances.  The F1 is a host expression over the counts: equal counts give bit-equal F1."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import capi
import layout_f1_restatement as R
import loss_inputs
import test_parse_quads as TQ
from test_gpu_detect import Buf

pytestmark = pytest.mark.gpu
GUARD = 1e-6


def run_kernel(sc, per_scene=True, acc=None):
    """one launch on a scene dict of the restatement's generators -> the (b, 4) rows (None without per_scene); acc: a Buf of
    five int64 that is incremented"""
    b, k = sc["verts4"].shape[:2]
    g, h = sc["gt_verts4"].shape[1], sc["horizontal"].shape[1]
    cols = sc["num_total"].shape[1]
    dev = {n: torch.from_numpy(np.ascontiguousarray(sc[n])).cuda() for n in ("count_f1", "verts4", "gt_verts4", "num_total",
                                                                              "horizontal")}
    rows = Buf((b, 4), torch.int32) if per_scene else None
    capi.ok("omnipq_layout_f1", b, k, capi.P(dev["count_f1"]), capi.P(dev["verts4"] if k else None), g,
            capi.P(dev["gt_verts4"] if g else None), capi.P(dev["num_total"] if g else None), cols, h,
            capi.P(dev["horizontal"] if h else None), ctypes.c_double(sc.get("same_thres", R.SAME_THRES)),
            capi.P(rows.t if rows else None), capi.P(acc.t if acc else None))
    torch.cuda.synchronize()
    assert (rows is None or rows.intact()) and (acc is None or acc.intact())
    return None if rows is None else rows.numpy()


def restated(sc, on_threshold=False):
    seen = []
    want = R.layout_f1_scene(sc, seen=seen)
    d = np.asarray(seen, np.float64)
    d = d[np.isfinite(d)]
    if not on_threshold:
        assert d.size == 0 or np.abs(d - sc.get("same_thres", R.SAME_THRES)).min() > GUARD
    return want


def variant(b, k, g, i):
    """call i of a shape: the quad counts 0, 1, 2, k and one beyond k rotate over the scenes and calls; num_total_cols 1 and
    256; h 0 and 4; in call 1 every list is empty (num_total 0), scene 0 of the others has all g rows; call 3 holds NaNs"""
    cols, h = (1, 256)[i % 2], (0, 4)[(i // 2) % 2]
    counts = [(0, 1, 2, k, k + 3)[(i + s) % 5] for s in range(b)]
    sc = R.random_scenes(1000 * k + 10 * g + i, b, k, g, cols=cols, h=h, counts=counts)
    if i == 1:
        sc["num_total"][:] = 0
    if i == 3:
        sc["verts4"][0, 0, 1, 2] = np.nan
        sc["gt_verts4"][0, 0, 2, 0] = np.nan
        if k > 1:
            sc["verts4"][0, 1] = np.inf
    return sc


@pytest.mark.parametrize("b,k,g", [(1, 1, 1), (2, 2, 32), (3, 64, 7), (1, 65, 32), (2, 256, 32), (1, 257, 5), (1, 4096, 32)])
def test_kernel_against_the_restatement_row_by_row(b, k, g):
    acc = Buf((5,), torch.int64, fill=0)
    total = np.zeros(5, np.int64)
    seen_counts, listed = set(), set()
    for i in range(5):
        sc = variant(b, k, g, i)
        want = restated(sc)
        got = run_kernel(sc, acc=acc)
        assert got.dtype == want.dtype and np.array_equal(got, want), (i, got.tolist(), want.tolist())
        assert np.array_equal(got[:, 0] + got[:, 1], np.clip(sc["count_f1"], 0, k))
        total += np.concatenate([want.sum(0), [b]])
        seen_counts |= set(int(c) for c in sc["count_f1"])
        listed |= set(int(n) for n in want[:, 2])
        if i == 2:
            assert np.array_equal(run_kernel(sc), got)                                   # two runs, the same bits
            before = acc.numpy().copy()
            assert run_kernel(sc, per_scene=False, acc=acc) is None                      # the accumulator alone
            assert np.array_equal(acc.numpy() - before, np.concatenate([want.sum(0), [b]]))
            total += np.concatenate([want.sum(0), [b]])
    assert np.array_equal(acc.numpy(), total)        # the sum of every call's per-scene rows, and the scans
    assert {0, 1, 2, k, k + 3} <= seen_counts
    assert {0, g} <= listed
    assert total[0] > 0 or k * b < 4                 # correct quads do occur


def test_two_quad_scenes_score_their_ceiling_and_floor():
    sc = R.random_scenes(**dict(FAMILY, family="two_quads"))
    want = restated(sc)
    assert 0 < want[:, 3].sum() < 2 * FAMILY["b"]
    assert np.array_equal(run_kernel(sc), want)


FAMILY = dict(seed=23, b=8, k=4, g=5, cols=1)        # tests/test_layout_f1_restatement.py: the host calculator agrees on it


@pytest.mark.parametrize("name", sorted(R.MERGE_CASES))
def test_merge_cases(name):
    for shift, tp_h in ((0.125, 2), (0.5, 0)):
        sc = R.merge_scene(name, shift)
        want = restated(sc)
        assert want[0, 3] == tp_h
        assert np.array_equal(run_kernel(sc), want)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_kernel_sides_with_the_rule_on_every_mutant_input(mutant):
    sc = R.mutant_input(mutant)
    want = restated(sc, on_threshold=(mutant == "strict"))
    assert not np.array_equal(want, R.layout_f1_scene(sc, mutant=mutant))
    assert np.array_equal(run_kernel(sc), want)


def test_exactly_representable_distances_at_the_threshold():
    assert run_kernel(R.boundary_scene(True)).tolist() == [[1, 0, 1, 0]]
    assert run_kernel(R.boundary_scene(False)).tolist() == [[0, 1, 1, 0]]
    sc = dict(R.boundary_scene(True), same_thres=0.0)                      # a threshold of zero: only equal corners pass
    assert run_kernel(sc).tolist() == [[0, 1, 1, 0]]
    sc["verts4"] = sc["gt_verts4"].copy()
    assert run_kernel(sc).tolist() == [[1, 0, 1, 0]]


def test_an_empty_batch_launches_nothing():
    null = capi.P(None)
    capi.ok("omnipq_layout_f1", 0, 256, null, null, 32, null, null, 1, 4, null, ctypes.c_double(0.4), null, null)


# ------------------------------------------------------------------------------------------------------ end to end
def golden_on_device(name):
    return {k: torch.from_numpy(v).cuda() for k, v in TQ.case_inputs(name).items()}


def host_calculator(det, ep, f1="host"):
    """the parent's route on the same record: to_lists(), parse_quad_groundtruths, QUADAPCalculator.step"""
    import ap_helper_pq
    calc = ap_helper_pq.QUADAPCalculator(0.25, {1: "quad"}, f1=f1)
    pred_map, _, corners = det.to_host().to_lists()
    gt_map, gt_corners = ap_helper_pq.parse_quad_groundtruths(ep, loss_inputs.EVAL_CONFIG)
    calc.step(pred_map, gt_map, corners, gt_corners, ep["horizontal_quads"])
    return calc


@pytest.mark.parametrize("name", TQ.CASES)
def test_layout_f1_step_gives_the_golden_f1_and_the_host_calculators_counts(name):
    import ap_helper_pq
    ep = golden_on_device(name)
    det = ap_helper_pq.detect_quad_predictions(ep, loss_inputs.EVAL_CONFIG, "last_")
    scorer = ap_helper_pq.LayoutF1("cuda:0")
    assert scorer.acc.dtype == torch.int64 and tuple(scorer.acc.shape) == (5,) and scorer.read()["scans"] == 0
    scorer.step(det, ep)
    plain, calculated = float(TQ.GOLD[f"{name}.f1_plain"][0]), float(TQ.GOLD[f"{name}.f1_calculated"][0])
    assert scorer.f1() == pytest.approx(plain, abs=1e-12)
    assert scorer.f1(calculated=True) == pytest.approx(calculated, abs=1e-12)
    counts = scorer.read()
    assert sorted(counts) == sorted(ap_helper_pq.F1_KEYS) and all(type(v) is int for v in counts.values())
    # the host calculator on to_lists() of the same record: the same counts, so the same bits
    host = host_calculator(det, ep)
    assert counts["scans"] == host.scan_cnt == det.B
    assert counts["npos"] == sum(len(host.gt_corners[i]) for i in range(host.scan_cnt))
    assert counts["tp_wall"] + counts["fp"] == sum(len(host.pred_corners[i]) for i in range(host.scan_cnt))
    assert host.compute_F1(calculated=False) == scorer.f1(False) and host.compute_F1(calculated=True) == scorer.f1(True)
    assert counts["tp_horizontal"] > 0 and counts["tp_wall"] > 0
    # the lists through the same kernel
    device = host_calculator(det, ep, f1="device")
    assert device.f1_counts_device() == counts
    for c in (False, True):
        assert device.compute_F1(calculated=c) == host.compute_F1(calculated=c)
    m_dev, m_host = device.compute_metrics(), host.compute_metrics()                   # untouched by the F1 route
    assert sorted(m_dev) == sorted(m_host) and all(np.array_equal(m_dev[k], m_host[k], equal_nan=True) for k in m_host)
    # a second step doubles every count; reset() clears them
    scorer.step(det, ep)
    assert scorer.read() == {k: 2 * v for k, v in counts.items()}
    scorer.reset()
    assert not any(scorer.read().values())


def test_device_route_refuses_corners_that_float32_cannot_hold():
    import ap_helper_pq
    ep = golden_on_device(TQ.CASES[0])
    det = ap_helper_pq.detect_quad_predictions(ep, loss_inputs.EVAL_CONFIG, "last_")
    calc = host_calculator(det, ep, f1="device")
    calc.pred_corners[0] = [np.asarray(q, np.float64) for q in calc.pred_corners[0]]          # wider, the same values: fine
    want = host_calculator(det, ep).compute_F1(calculated=True)
    assert calc.compute_F1(calculated=True) == want
    calc.pred_corners[0][0] = calc.pred_corners[0][0] + 1e-12
    with pytest.raises(ValueError, match="not exactly representable in float32"):
        calc.compute_F1()
    calc.f1 = "host"
    assert calc.compute_F1(calculated=True) == want                                        # the host route takes them


def test_a_second_step_allocates_nothing_and_labels_of_other_types_are_staged():
    import ap_helper_pq
    ep = golden_on_device(TQ.CASES[0])
    det = ap_helper_pq.detect_quad_predictions(ep, loss_inputs.EVAL_CONFIG, "last_")
    odd = dict(ep, gt_quad_centers=torch.cat([ep["gt_quad_centers"].double(), ep["gt_quad_centers"].double()], dim=2),
               num_total_quads=ep["num_total_quads"][:, 0].int(), gt_quad_sizes=ep["gt_quad_sizes"].double())
    for labels in (ep, odd):
        scorer = ap_helper_pq.LayoutF1("cuda:0")
        first = scorer.step(det, labels).read()
        torch.cuda.synchronize()
        stats, held = torch.cuda.memory_stats(), torch.cuda.memory_allocated()
        scorer.step(det, labels)
        after = torch.cuda.memory_stats()
        assert after["allocation.all.allocated"] == stats["allocation.all.allocated"]
        assert torch.cuda.memory_allocated() == held
        assert scorer.read() == {k: 2 * v for k, v in first.items()}
    assert first == ap_helper_pq.LayoutF1("cuda:0").step(det, ep).read()                   # staged labels, the same counts
    with pytest.raises(RuntimeError, match="reads nothing from the host"):
        ap_helper_pq.LayoutF1("cuda:0").step(det, dict(ep, horizontal_quads=ep["horizontal_quads"].cpu()))
    boxes_like = ap_helper_pq.Detections("boxes", 1, 4, torch.device("cuda", 0), ncls=2, ns=2)
    with pytest.raises(ValueError, match="quad record"):
        ap_helper_pq.LayoutF1("cuda:0").step(boxes_like, ep)


def test_step_under_capture_adds_the_counts_of_the_batch_it_is_replayed_on():
    import ap_helper_pq
    cfg = loss_inputs.EVAL_CONFIG
    first = TQ.case_inputs(TQ.CASES[0])
    B, KQ = first["last_quad_scores"].shape[:2]
    second = loss_inputs.make_eval(91, B=B, KQ=KQ, two_walls_scene=False)
    ep = {k: torch.from_numpy(v).cuda() for k, v in first.items()}
    det = ap_helper_pq.detect_quad_predictions(ep, cfg, "last_")
    scorer = ap_helper_pq.LayoutF1("cuda:0")
    one = scorer.step(det, ep).read()                # eager: the buffers exist from here on
    torch.cuda.synchronize()
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scorer.step(det, ep)
    scorer.reset()
    graph.replay()
    assert scorer.read() == one                      # the batch it was captured on
    for k in ep:
        ep[k].copy_(torch.from_numpy(second[k]))
    ap_helper_pq.detect_quad_predictions(ep, cfg, "last_", out=det)
    graph.replay()
    two = ap_helper_pq.LayoutF1("cuda:0").step(det, {k: v.clone() for k, v in ep.items()}).read()
    assert two != one and two["npos"] > 0 and two["tp_wall"] + two["fp"] > 0
    assert scorer.read() == {k: one[k] + two[k] for k in one}


# ------------------------------------------------------------------------------------------------------ the runner
@pytest.fixture(scope="module")
def world():
    """the model and batches of tests/test_gpu_captured_inference.py, three of them, each with quad labels made from the
    runner's own predictions for it: the ground truth of a scene is its F1 list's first quads but the last one, so correct
    quads, false positives and unmatched ground truth all occur"""
    import inference
    import synth
    import test_gpu_captured_inference as TC
    from pq_transformer import PQ_Transformer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = PQ_Transformer(input_feature_dim=1, num_class=18, num_proposal=256, num_quad_proposal=256, num_heading_bin=1,
                         num_size_cluster=18, mean_size_arr=TC.MEANS).to(dev).eval()
    cfg = TC.config()
    clouds = []
    for seed in (81, 82, 83):
        cloud = synth.make_clouds(seed, 2, 4096, kind="room").to(dev)
        clouds.append(torch.cat([cloud[..., :3], cloud[..., 2:3]], dim=2).contiguous())
    runner = inference.CapturedInference(net, clouds[0], cfg, objects=True, quads=True)
    batches = []
    for pc in clouds:
        quads = runner.run(pc)["last_"][1]
        idx = quads.index_f1.long().clamp(min=0)[:, :32]
        ep = runner.end_points

        def take(t):
            return torch.gather(t.float(), 1, idx[..., None].expand(-1, -1, t.shape[-1])).contiguous()

        n = (quads.count_f1.long().clamp(max=32) - 1).clamp(min=0)
        hz = torch.zeros((2, 4, 4, 3), device=dev)
        batches.append({"point_clouds": pc, "gt_quad_centers": take(ep["last_quad_center"]),
                        "gt_normal_vectors": take(ep["last_normal_vector"]), "gt_quad_sizes": take(ep["last_quad_size"]),
                        "num_gt_quads": n[:, None].repeat(1, 256), "num_total_quads": n[:, None].repeat(1, 256),
                        "horizontal_quads": hz})
    torch.cuda.synchronize()
    return runner, batches, cfg


def test_evaluate_layout_f1_equals_the_host_route_on_the_same_records(world):
    import ap_helper_pq
    import inference
    runner, batches, cfg = world
    host = ap_helper_pq.QUADAPCalculator(0.25, {1: "quad"})
    for batch in batches:                            # the parent's route: run(), to_lists(), step
        quads = runner.run(batch)["last_"][1]
        pred_map, _, corners = quads.to_lists()
        gt_map, gt_corners = ap_helper_pq.parse_quad_groundtruths(batch, cfg)
        host.step(pred_map, gt_map, corners, gt_corners, batch["horizontal_quads"])
    replays = runner.replays
    scorer = inference.evaluate_layout_f1(runner, batches)
    assert isinstance(scorer, ap_helper_pq.LayoutF1) and runner.replays == replays + 3
    counts = scorer.read()
    print("evaluate_layout_f1 counts:", counts)
    assert counts["scans"] == 6 and counts["npos"] == sum(len(host.gt_corners[i]) for i in range(6))
    assert counts["tp_wall"] + counts["fp"] == sum(len(host.pred_corners[i]) for i in range(6))
    assert counts["tp_wall"] > 0 and counts["npos"] > 0
    for c in (False, True):
        assert scorer.f1(calculated=c) == host.compute_F1(calculated=c)
    host.f1 = "device"
    assert host.f1_counts_device() == counts
    with pytest.raises(ValueError, match="no quad record"):
        inference.evaluate_layout_f1(runner, batches, prefix="proposal_")


def test_run_without_to_host_leaves_the_pinned_twins_untouched(world):
    runner, batches, cfg = world
    boxes, quads = runner.run(batches[0])["last_"]
    quads.host_fields(), boxes.host_fields()         # waits for both copies
    twins = quads._host.clone(), boxes._host.clone()
    record = quads.record.clone()
    again = runner.run(batches[1], to_host=False)["last_"]
    torch.cuda.synchronize()
    assert again[0] is boxes and again[1] is quads
    assert not torch.equal(quads.record, record)                                           # another batch on the device ...
    assert torch.equal(quads._host, twins[0]) and torch.equal(boxes._host, twins[1])       # ... and not on the host
    runner.run(batches[1])
    quads.host_fields()
    assert not torch.equal(quads._host, twins[0])
