"""Host half of the device route of the detection metrics: the C entry points' validation, the packing of the
calculators' lists into segments, and the greedy match from per-detection best overlaps -- which must return what
eval_det_cls's loop returns, array for array.  Nothing here needs a GPU: the best overlaps are computed on the host with
eval_det.box3d_iou and the loop's own rule."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (sys.path set-up)
import loss_inputs
import test_parse_boxes
import test_parse_quads

EINVAL, ETOOLARGE = 10001, 10002


def test_entry_points_validate_before_touching_the_device(built_lib):
    import capi
    lib = capi.lib()
    p, null, ll = ctypes.c_void_p(0x1000), ctypes.c_void_p(0), ctypes.c_longlong        # p is never dereferenced
    pairs, best = lib.omnipq_obb_iou_pairs, lib.omnipq_obb_iou_best
    assert pairs(ll(-1), p, p, p, p, null) == EINVAL
    assert pairs(ll(5), null, p, p, p, null) == EINVAL
    assert pairs(ll(5), p, null, p, p, null) == EINVAL
    assert pairs(ll(5), p, p, null, null, null) == EINVAL                               # either output, not neither
    assert pairs(ll(1 << 31), p, p, p, null, null) == ETOOLARGE
    assert pairs(ll(0), null, null, null, null, null) == 0
    assert pairs(ll(0), p, p, p, p, null) == 0

    def call(n_pred=5, pred8=p, pred_seg=p, n_seg=2, seg_start=p, n_gt=7, gt8=p, ovmax=p, jmax=p):
        return best(ll(n_pred), pred8, pred_seg, n_seg, seg_start, ll(n_gt), gt8, ovmax, jmax, null)

    assert call(n_pred=-1) == EINVAL and call(n_gt=-1) == EINVAL and call(n_seg=-1) == EINVAL
    assert call(n_seg=0) == EINVAL                                                      # detections without a segment table
    for name in ("pred8", "pred_seg", "seg_start", "gt8", "ovmax", "jmax"):
        assert call(**{name: null}) == EINVAL, name
    assert call(n_pred=1 << 31) == ETOOLARGE and call(n_gt=1 << 31) == ETOOLARGE
    assert call(n_pred=0) == 0
    assert call(n_pred=0, pred8=null, pred_seg=null, n_seg=0, seg_start=null, n_gt=0, gt8=null, ovmax=null, jmax=null) == 0


def box(cx, cz, w=1.0, d=1.0, y0=0.0, y1=1.0, ang=0.0):
    """corners (8, 3) in get_3d_box's layout (rows 0-3 the top face, up = -Y) of a box over the footprint centre (cx, cz)"""
    c, s = np.cos(ang), np.sin(ang)
    x = np.array([w, w, -w, -w]) / 2
    z = np.array([d, -d, -d, d]) / 2
    fx, fz = c * x + s * z + cx, -s * x + c * z + cz
    return np.stack([np.concatenate([fx, fx]), np.array([y1] * 4 + [y0] * 4), np.concatenate([fz, fz])], 1)


def host_pairs(a, b):
    import eval_det
    got = np.array([eval_det.box3d_iou(x, y) for x, y in zip(a, b)])
    return got[:, 0], got[:, 1]


def degenerate_pairs():
    q = np.pi / 4
    cases = [
        (box(0, 0), box(0, 0)),                                                  # identical
        (box(0.3, -0.2, 1.2, 0.7, ang=0.7), box(0.3, -0.2, 1.2, 0.7, ang=0.7)),  # identical, rotated
        (box(0, 0, 2, 2), box(0.1, 0.1, 0.5, 0.5)),                              # one inside the other
        (box(0.1, 0.1, 0.5, 0.5), box(0, 0, 2, 2)),
        (box(0, 0, 2, 2), box(0.1, 0.1, 0.5, 0.5, ang=0.4)),
        (box(0, 0), box(5, 5)),                                                  # disjoint
        (box(0, 0, ang=0.3), box(5, 5, ang=1.1)),
        (box(0, 0), box(1, 0)),                                                  # sharing an edge
        (box(0, 0), box(0, -1)),
        (box(0, 0), box(1, 1)),                                                  # sharing only a vertex
        (box(0, 0, ang=q), box(np.sqrt(2.0), 0, ang=q)),
        (box(0, 0, y0=0, y1=1), box(0, 0, y0=2, y1=3)),                          # the same footprint, disjoint heights
        (box(0, 0, y0=0, y1=1), box(0, 0, y0=1, y1=2)),                          # heights touching
        (box(0, 0, y0=0, y1=1), box(0.2, 0.1, y0=0.5, y1=2)),
        (box(0, 0), box(0.3, 0.2, 1.5, 0.7)),                                    # axis-aligned against axis-aligned
        (box(1, 2, 0.8, 2.5), box(1.2, 1.0, 2.0, 0.9, y0=0.3, y1=0.8)),
        (box(0, 0), box(0.5, 0.5)),
        (box(0, 0), box(0.2, 0.1, ang=q)),                                       # 45 degrees
        (box(0, 0, ang=q), box(0, 0)),
        (box(0, 0), box(0, 0, ang=1e-3)),                                        # 1e-3 rad
        (box(0, 0, ang=q), box(0.1, 0, ang=q + 1e-3)),
        (box(0.4, 0.3, 1.3, 0.9, ang=-1e-3), box(0.4, 0.3, 1.3, 0.9, ang=1e-3)),
        (box(0, 0, 2, 0.1), box(0, 0, 0.1, 2)),                                  # 0.1-thick quads crossing at right angles
        (box(0.5, 0.2, 2, 0.1, y1=2.5, ang=0.3), box(0.4, 0.3, 2, 0.1, y1=2.5, ang=0.3 + np.pi / 2)),
        (box(0, 0, 3, 0.1, ang=q), box(0.2, 0.2, 0.1, 3, ang=q)),
    ]
    a, b = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    return a, b, host_pairs(a, b)


def same(a, b):
    """equal, a NaN (a class without ground truth divides by zero, here as there) equal to a NaN"""
    return np.array_equal(a, b, equal_nan=True)


def same_metrics(a, b):
    return list(a) == list(b) and all(same(a[k], b[k]) for k in a)


def host_lists_equal(pred_all, gt_all, thresholds=(0.25, 0.5)):
    """pack_segments + the loop's best overlaps on the host + match_from_best == eval_det, per class and threshold"""
    import eval_det
    pack = eval_det.pack_segments(pred_all, gt_all)
    ovmax, jmax = eval_det.best_on_host(pack)
    for thr in thresholds:
        want = eval_det.eval_det(pred_all, gt_all, ovthresh=thr)
        got = eval_det.eval_from_best(pack, ovmax, jmax, thr)
        assert list(got[2]) == list(want[2])                                           # the classes, in eval_det's order
        for cls in want[2]:
            assert same(got[0][cls], want[0][cls]), (thr, cls)
            assert same(got[1][cls], want[1][cls]), (thr, cls)
            assert same(got[2][cls], want[2][cls]) and np.ndim(got[2][cls]) == 0, (thr, cls)
    return pack, ovmax, jmax


def hand_case():
    """3 scans.  Class 7 occurs only in the predictions (empty segments), class 9 only in the ground truth (no segment, scored
    0), scan 2 has no predictions, two detections of class 3 in different scans have equal scores."""
    pred_all = {0: [(3, box(0, 0), 0.9), (7, box(5, 5), 0.8), (3, box(0.1, 0), 0.5), (3, box(3, 3), 0.7)],
                1: [(3, box(1, 1), 0.7), (7, box(2, 2), 0.6), (3, box(9, 9), 0.3)],
                2: []}
    gt_all = {0: [(3, box(0, 0.05)), (9, box(4, 4)), (3, box(3, 3.2))],
              1: [(3, box(1.1, 1))],
              2: [(3, box(0, 0)), (9, box(1, 1))]}
    return pred_all, gt_all


def test_pack_segments_on_a_hand_written_case():
    import eval_det
    pred_all, gt_all = hand_case()
    pack, ovmax, jmax = host_lists_equal(pred_all, gt_all)
    assert pack["classes"] == [3, 7, 9]                                                # gt's insertion order
    assert pack["per_class"][9] is None                                                # ground truth only: no segment
    c3, c7 = pack["per_class"][3], pack["per_class"][7]
    # the order of eval_det_cls's `dets`: scan by scan in the order the class's predictions arrived
    assert c3["img"] == [0, 0, 0, 1, 1] and list(c3["conf"]) == [0.9, 0.5, 0.7, 0.7, 0.3] and c3["npos"] == 4
    assert c7["img"] == [0, 1] and list(c7["conf"]) == [0.8, 0.6] and c7["npos"] == 0
    assert (c3["lo"], c3["hi"], c7["lo"], c7["hi"]) == (0, 5, 5, 7)
    want_boxes = [box(0, 0), box(0.1, 0), box(3, 3), box(1, 1), box(9, 9), box(5, 5), box(2, 2)]
    assert np.array_equal(pack["pred8"], np.stack(want_boxes)) and pack["pred8"].dtype == np.float64
    # segments: (3, scan 0) with two boxes, (3, scan 1) with one, (7, scan 0) and (7, scan 1) empty; scan 2's ground truth of
    # class 3 belongs to no segment (nothing is matched against it) but counts in npos
    assert pack["pred_seg"].tolist() == [0, 0, 0, 1, 1, 2, 3] and pack["pred_seg"].dtype == np.int32
    assert pack["seg_start"].tolist() == [0, 2, 3, 3, 3] and pack["seg_start"].dtype == np.int64
    assert np.array_equal(pack["gt8"], np.stack([box(0, 0.05), box(3, 3.2), box(1.1, 1)]))
    for cls in (3, 7):
        c = pack["per_class"][cls]
        assert np.array_equal(c["seg"], pack["pred_seg"][c["lo"]:c["hi"]])
    assert jmax[:4].tolist() == [0, 0, 1, 0] and np.isinf(ovmax[5:]).all() and (jmax[5:] == -1).all()
    assert ovmax[4] == 0.0 and jmax[4] == 0                                            # overlaps nothing: the first box
    # the two detections scoring 0.7 fall as np.argsort(-conf) lets them fall in eval_det_cls
    rec, prec, ap = eval_det.match_from_best(c3["conf"], c3["seg"], ovmax[:5], jmax[:5], c3["npos"], 0.25)
    want = eval_det.eval_det_cls({0: [(b, s) for c, b, s in pred_all[0] if c == 3], 1: [(b, s) for c, b, s in pred_all[1] if c == 3]},
                                 {0: [b for c, b in gt_all[0] if c == 3], 1: [b for c, b in gt_all[1] if c == 3],
                                  2: [b for c, b in gt_all[2] if c == 3]}, 0.25)
    assert np.array_equal(rec, want[0]) and np.array_equal(prec, want[1]) and ap == want[2]
    assert rec[-1] == 0.75                                                             # three of the four boxes found


def test_pack_segments_of_nothing():
    import eval_det
    pack = eval_det.pack_segments({}, {})
    assert pack["classes"] == [] and pack["pred8"].shape == (0, 8, 3) and pack["gt8"].shape == (0, 8, 3)
    assert pack["seg_start"].tolist() == [0] and len(pack["pred_seg"]) == 0
    assert eval_det.eval_from_best(pack, np.zeros(0), np.zeros(0, np.int32), 0.25) == ({}, {}, {})


def as_dicts(pred_map, gt_map):
    return dict(enumerate(pred_map)), dict(enumerate(gt_map))


@pytest.mark.parametrize("name", ["a", "b"])
def test_match_from_best_equals_the_loop_on_the_golden_quads(name):
    ep = test_parse_quads.case_inputs(name)
    pred_map, _, _, gt_map, _ = test_parse_quads.oracle_parse(ep, loss_inputs.EVAL_CONFIG)
    host_lists_equal(*as_dicts(pred_map, gt_map))


@pytest.mark.parametrize("name", sorted(test_parse_boxes.MODES))
def test_match_from_best_equals_the_loop_on_the_golden_boxes(name):
    cfg = loss_inputs.eval_config(**test_parse_boxes.MODES[name])
    pred_map, _, gt_map = test_parse_boxes.oracle_parse(test_parse_boxes.inputs(), cfg)
    host_lists_equal(*as_dicts(pred_map, gt_map))


def ragged_accumulation(seed, scans=6, classes=4):
    """Rotated random boxes with duplicate ground-truth boxes, duplicate scores, a prediction-only class, a
    ground-truth-only class and scans without predictions."""
    rs = np.random.RandomState(seed)

    def rbox():
        return box(*(rs.rand(2) * 2.0), w=0.4 + rs.rand(), d=0.4 + rs.rand(), y0=rs.rand() * 0.3, y1=0.6 + rs.rand() * 0.5,
                   ang=rs.rand() * 2 * np.pi)

    pred_all, gt_all = {}, {}
    for img in range(scans):
        gts = [(int(rs.randint(classes)), rbox()) for _ in range(rs.randint(0, 7))]
        if gts:
            gts.append((gts[0][0], gts[0][1].copy()))                                  # an exact duplicate, later in the list
        gts += [(classes + 1, rbox())] * (img % 2)                                     # a class no prediction has
        gt_all[img] = gts
        preds = []
        if img != 2:                                                                   # a scan without predictions
            for _ in range(rs.randint(3, 14)):
                score = float(np.round(rs.rand(), 1))                                  # 11 values: many equal scores
                preds.append((int(rs.randint(classes)), rbox(), np.float32(score)))
            for c, g in gts[:3]:                                                       # some close to the ground truth
                preds.append((c, g + rs.randn(1, 3) * 0.02, np.float32(np.round(rs.rand(), 1))))
            preds.append((classes, rbox(), np.float32(0.5)))                           # a class no ground truth has
        pred_all[img] = preds
    return pred_all, gt_all


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_match_from_best_equals_the_loop_on_duplicates(seed):
    pred_all, gt_all = ragged_accumulation(seed)
    pack, ovmax, jmax = host_lists_equal(pred_all, gt_all, thresholds=(0.25, 0.5, 0.0))
    assert (ovmax > 0.5).sum() >= 5 and np.isinf(ovmax).any()
    confs = np.concatenate([c["conf"] for c in pack["per_class"].values() if c is not None])
    assert len(np.unique(confs)) < len(confs) // 2                                     # equal scores did occur


def test_calculators_refuse_an_unknown_route(built_lib):
    import ap_helper_pq
    for make in (ap_helper_pq.APCalculator, ap_helper_pq.QUADAPCalculator):
        assert make(0.25, None).iou == "host" and make(0.25, None, iou="device").iou == "device"
        with pytest.raises(ValueError, match="bogus"):
            make(0.25, None, iou="bogus")


def test_host_calculators_at_several_thresholds_equal_one_calculator_each(built_lib):
    import ap_helper_pq
    pred_all, gt_all = ragged_accumulation(3)
    calcs = {t: ap_helper_pq.APCalculator(t, None) for t in (0.25, 0.5)}
    for c in calcs.values():
        c.step(list(pred_all.values()), list(gt_all.values()))
    both = ap_helper_pq.compute_metrics_at(calcs[0.25], (0.25, 0.5))
    assert same_metrics(both[0], calcs[0.25].compute_metrics()) and same_metrics(both[1], calcs[0.5].compute_metrics())
    assert not same_metrics(both[0], both[1])


def test_device_route_refuses_a_foreign_iou_function_and_the_cpu(built_lib):
    import torch
    import eval_det
    pred_all, gt_all = hand_case()
    with pytest.raises(ValueError, match="get_iou_obb"):
        eval_det.eval_det_device(pred_all, gt_all, get_iou_func=lambda a, b: 0.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        eval_det.box3d_iou_batch(torch.zeros(2, 8, 3, dtype=torch.float64), torch.zeros(2, 8, 3, dtype=torch.float64))
