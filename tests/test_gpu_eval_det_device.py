"""Device route of the detection metrics (csrc/eval_iou.hip) on the GPU: the oriented-box IoU elementwise against
the reference's samples and against eval_det.box3d_iou, the per-detection best match against eval_det_cls's loop, the two
calculators end to end against the reference's metrics, and eval_det_device against eval_det.

The bound 1e-12 is the one tests/test_parse_quads.py holds between eval_det.box3d_iou and the reference's values.  The kernel
restates the host's arithmetic operation for operation in f64 without contraction; only the order of the shoelace sums
differs, a few units of 2^-53 times the coordinate products (metres squared, below 100 here)."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import loss_inputs
import test_parse_boxes
import test_parse_quads
from test_eval_det_device_host import degenerate_pairs, host_pairs, ragged_accumulation, same, same_metrics

pytestmark = pytest.mark.gpu
TOL = 1e-12


def device_pairs(a, b):
    import eval_det
    i3, i2 = eval_det.box3d_iou_batch(torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                                      torch.from_numpy(np.ascontiguousarray(b)).cuda())
    return i3.cpu().numpy(), i2.cpu().numpy()


def test_pairs_against_the_reference_samples():
    gold = test_parse_quads.GOLD
    boxes = gold["iou.boxes"]
    ia = [i for i in range(0, 40, 2) for j in range(1, 40, 2)]
    ib = [j for i in range(0, 40, 2) for j in range(1, 40, 2)]
    i3, i2 = device_pairs(boxes[ia], boxes[ib])
    assert i3.shape == (400,) and (gold["iou.values"] > 0).sum() > 20
    print("iou3d against the reference:", np.abs(i3 - gold["iou.values"]).max())
    assert np.abs(i3 - gold["iou.values"]).max() <= TOL
    want3, want2 = host_pairs(boxes[ia], boxes[ib])
    print("iou3d, iou2d against the host:", np.abs(i3 - want3).max(), np.abs(i2 - want2).max())
    assert np.abs(i2 - want2).max() <= TOL and (want2 > 0).sum() > 20


@pytest.fixture(scope="module")
def degenerate():
    return degenerate_pairs()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_pairs_on_degenerate_geometry_against_the_host(degenerate, n):
    a, b, (want3, want2) = degenerate
    pick = (np.arange(n) * 7 + n + 1) % len(a)                                      # every case occurs from n = 63 on
    assert n < 63 or len(set(pick.tolist())) == len(a)
    i3, i2 = device_pairs(a[pick], b[pick])
    # The identical rotated pair is NaN on the host, as in the reference: an edge of the subject that lies on the clip edge
    # tests inside at one end and outside at the other by rounding, and the intersection of two parallel lines divides by
    # zero.  The kernel makes the same decisions and must say NaN there too, and nowhere else.
    nan = np.isnan(want3[pick])
    assert np.isnan(want3).sum() == 1 and np.array_equal(np.isnan(want2[pick]), nan)
    assert np.array_equal(np.isnan(i3), nan) and np.array_equal(np.isnan(i2), nan)
    err3, err2 = np.abs(i3 - want3[pick])[~nan], np.abs(i2 - want2[pick])[~nan]
    print(n, err3.max(initial=0.0), err2.max(initial=0.0))
    assert err3.max(initial=0.0) <= TOL and err2.max(initial=0.0) <= TOL
    # zero where it is zero on the host (disjoint, a shared edge or vertex, disjoint or touching heights), one where identical
    assert np.array_equal(i3 == 0, want3[pick] == 0) and np.array_equal(i2 == 0, want2[pick] == 0)
    # each output alone (the other NULL) gives the same bits
    import ctypes
    import capi
    ta, tb = torch.from_numpy(a[pick]).cuda(), torch.from_numpy(b[pick]).cuda()
    only3, only2 = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    capi.ok("omnipq_obb_iou_pairs", ctypes.c_longlong(n), capi.P(ta), capi.P(tb), capi.P(only3), capi.P(None))
    capi.ok("omnipq_obb_iou_pairs", ctypes.c_longlong(n), capi.P(ta), capi.P(tb), capi.P(None), capi.P(only2))
    assert same(only3.cpu().numpy(), i3) and same(only2.cpu().numpy(), i2)


RAGGED_SEED = 1                                      # chosen on the CPU: check_ragged_host_values holds, smallest gap 2.6e-5
SEG_SIZES = (0, 1, 2, 33, 64, 65)                    # ground-truth boxes per segment
SEG_DETS = (100, 1, 400, 250, 150, 99)               # detections per segment: 1000, one segment with a single one


def ragged_best_case():
    """-> pred8, pred_seg, seg_start, gt8 and the host loop's (all overlaps per detection, ovmax, jmax)"""
    import eval_det
    from oracle import ap_oracle
    rs = np.random.RandomState(RAGGED_SEED)

    def rotated(n):                                  # as tests/golden/make_golden_parse_quads.py builds its IoU samples
        c = (rs.rand(1, n, 3) * 2).astype(np.float32)
        nv = rs.randn(1, n, 3).astype(np.float32)
        s = (0.5 + rs.rand(1, n, 2)).astype(np.float32)
        return ap_oracle.decode_quads(c, nv, s, length=0.6)[0][0]

    seg_start = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int64)
    gt8 = rotated(int(seg_start[-1]))
    gt8[seg_start[3] + 32] = gt8[seg_start[3] + 5]                               # exact duplicates at a later index
    gt8[seg_start[5] + 64] = gt8[seg_start[5] + 10]
    pred8 = rotated(sum(SEG_DETS))
    pred_seg = np.repeat(np.arange(len(SEG_SIZES)), SEG_DETS).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(SEG_DETS)])
    for s, j in ((3, 5), (5, 10)):                                               # detections whose best box is the duplicated one
        for t in range(6):
            pred8[first[s] + t] = gt8[seg_start[s] + j] + rs.randn(1, 3) * 0.01
    for s in (2, 3, 4, 5):                                                       # detections that overlap nothing
        pred8[first[s] + 20:first[s] + 25] += 100.0
    pred8[first[1]] = gt8[seg_start[1]] + 0.05                                   # the single detection of its segment
    perm = np.concatenate([rs.permutation(np.arange(first[s], first[s + 1])) for s in range(len(SEG_SIZES))])
    pred8 = pred8[perm]
    overlaps = [np.array([eval_det.get_iou_obb(pred8[i], gt8[j]) for j in range(seg_start[s], seg_start[s + 1])])
                for i, s in enumerate(pred_seg)]
    ovmax, jmax = np.full(len(pred8), -np.inf), np.full(len(pred8), -1, dtype=np.int32)
    for i, ov in enumerate(overlaps):
        for j, v in enumerate(ov):
            if v > ovmax[i]:
                ovmax[i], jmax[i] = v, j
    return pred8, pred_seg, seg_start, gt8, overlaps, ovmax, jmax


def check_ragged_host_values(pred_seg, overlaps, ovmax, jmax):
    """What the case promises, on the host values alone: the features are there, and the best overlap exceeds every other
    one that is not bit-equal to it by more than 1e-9, so that 1e-12 of error cannot change an index."""
    gaps = [ovmax[i] - ov[ov != ovmax[i]].max() for i, ov in enumerate(overlaps) if (ov != ovmax[i]).any()]
    assert min(gaps) > 1e-9, min(gaps)
    dup = [i for i, ov in enumerate(overlaps) if ovmax[i] > 0 and (ov == ovmax[i]).sum() == 2]
    assert {int(pred_seg[i]) for i in dup} == {3, 5} and len(dup) >= 12
    assert all(jmax[i] in (5, 10) for i in dup)                                  # the earlier of the two
    nothing = (ovmax == 0) & (jmax == 0)
    assert nothing.sum() >= 20 and set(pred_seg[nothing].tolist()) >= {2, 3, 4, 5}
    assert (np.isinf(ovmax) == (pred_seg == 0)).all() and (jmax[pred_seg == 0] == -1).all()
    assert (pred_seg == 1).sum() == 1 and ovmax[pred_seg == 1][0] > 0.25
    assert (ovmax > 0.25).sum() > 200 and len(np.unique(jmax[pred_seg == 5])) > 30
    return min(gaps)


def test_best_match_on_ragged_segments_against_the_host_loop():
    import ctypes
    import capi
    pred8, pred_seg, seg_start, gt8, overlaps, want_ov, want_j = ragged_best_case()
    print("smallest gap between the best overlap and the runner-up:", check_ragged_host_values(pred_seg, overlaps, want_ov, want_j))
    n = len(pred8)
    t = [torch.from_numpy(x).cuda() for x in (pred8, pred_seg, seg_start, gt8)]
    ovmax = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    jmax = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    capi.ok("omnipq_obb_iou_best", ctypes.c_longlong(n), capi.P(t[0]), capi.P(t[1]), len(SEG_SIZES), capi.P(t[2]),
            ctypes.c_longlong(len(gt8)), capi.P(t[3]), capi.P(ovmax), capi.P(jmax))
    got_ov, got_j = ovmax.cpu().numpy(), jmax.cpu().numpy()
    assert np.array_equal(np.isinf(got_ov), np.isinf(want_ov)) and (got_ov[np.isinf(got_ov)] < 0).all()
    finite = np.isfinite(want_ov)
    print("ovmax against the host loop:", np.abs(got_ov[finite] - want_ov[finite]).max())
    assert np.abs(got_ov[finite] - want_ov[finite]).max() <= TOL
    assert np.array_equal(got_j, want_j)
    # the product's own route over the same arrays: one upload, one launch, one download
    import eval_det
    pack = {"pred8": pred8, "pred_seg": pred_seg, "seg_start": seg_start, "gt8": gt8}
    ov2, j2 = eval_det.best_on_device(pack)
    assert np.array_equal(ov2, got_ov) and np.array_equal(j2, got_j)


def check_device_calculators(make, step, gold, head):
    """calculators with iou="device" at both thresholds against the reference's metrics (abs 1e-9, the bound of the host
    route's tests), and compute_metrics_at against the two single-threshold results"""
    import ap_helper_pq
    single = []
    for thr in (0.25, 0.5):
        calc = make(thr)
        assert calc.iou == "device"
        step(calc)
        metrics = calc.compute_metrics()
        keys = [k for k in gold.files if k.startswith(f"{head}metrics{thr}.")]
        assert keys
        for k in keys:
            assert float(metrics[k.rpartition(f"metrics{thr}.")[2]]) == pytest.approx(float(gold[k][0]), abs=1e-9), k
        single.append(metrics)
    both = ap_helper_pq.compute_metrics_at(calc, (0.25, 0.5))
    assert same_metrics(both[0], single[0]) and same_metrics(both[1], single[1])


@pytest.mark.parametrize("name", ["a", "b"])
def test_quad_calculator_on_the_device_route_reproduces_the_reference(name):
    import ap_helper_pq
    ep = {k: torch.from_numpy(v).cuda() for k, v in test_parse_quads.case_inputs(name).items()}
    pred_map, _, corners = ap_helper_pq.parse_quad_predictions(ep, loss_inputs.EVAL_CONFIG, "last_")
    gt_map, gt_corners = ap_helper_pq.parse_quad_groundtruths(ep, loss_inputs.EVAL_CONFIG)
    check_device_calculators(lambda thr: ap_helper_pq.QUADAPCalculator(thr, {1: "quad"}, iou="device"),
                             lambda calc: calc.step(pred_map, gt_map, corners, gt_corners, ep["horizontal_quads"]),
                             test_parse_quads.GOLD, f"{name}.")


@pytest.mark.parametrize("name", sorted(test_parse_boxes.MODES))
def test_box_calculator_on_the_device_route_reproduces_the_reference(name):
    import ap_helper_pq
    cfg = loss_inputs.eval_config(**test_parse_boxes.MODES[name])
    ep = {k: torch.from_numpy(v).cuda() for k, v in test_parse_boxes.inputs().items()}
    pred_map, _ = ap_helper_pq.parse_predictions(ep, cfg, "last_")
    gt_map = ap_helper_pq.parse_groundtruths(ep, cfg)
    check_device_calculators(lambda thr: ap_helper_pq.APCalculator(thr, None, iou="device"),
                             lambda calc: calc.step(pred_map, gt_map), test_parse_boxes.GOLD, f"{name}.")


def test_eval_det_device_equals_eval_det():
    import eval_det
    pred_all, gt_all = ragged_accumulation(0, scans=6, classes=4)
    triples = eval_det.eval_det_device(pred_all, gt_all, ovthresh=(0.25, 0.5))
    for thr, got in zip((0.25, 0.5), triples):
        want = eval_det.eval_det(pred_all, gt_all, ovthresh=thr)
        assert list(got[2]) == list(want[2]) and len(want[2]) == 6
        for cls in want[2]:
            assert same(got[0][cls], want[0][cls]) and same(got[1][cls], want[1][cls]), (thr, cls)
            assert same(got[2][cls], want[2][cls]), (thr, cls)
    one = eval_det.eval_det_device(pred_all, gt_all, ovthresh=0.5, get_iou_func=eval_det.get_iou_obb)
    assert all(same(one[0][c], triples[1][0][c]) and same(one[2][c], triples[1][2][c]) for c in one[2])
