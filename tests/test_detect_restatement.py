"""CPU: the float64 restatement of the packed detections (tests/detect_restatement.py) reproduces the outputs of the REFERENCE's
parse_predictions / parse_quad_predictions (tests/golden/parse_boxes.npz, parse_quads.npz) through the three modes of
test_parse_boxes.MODES, and each of its five mutants fails on an input built for it.  No library, no GPU."""
import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (sys.path set-up)
import detect_restatement as R
import loss_inputs
import test_parse_boxes as TB
import test_parse_quads as TQ


@pytest.mark.parametrize("name", sorted(TB.MODES))
def test_restated_boxes_reproduce_the_reference(name):
    """counts, classes, order and pred_mask exactly, scores within rtol 2e-6 / atol 1e-8, boxes within BOX_TOL: TB.check"""
    cfg = loss_inputs.eval_config(**TB.MODES[name])
    ep = TB.inputs()
    rec = R.detect_boxes(ep, cfg, "last_")
    pred_map, mask = R.boxes_to_lists(rec, cfg)
    gt_map = TB.oracle_parse(ep, cfg)[2]
    TB.check(name, cfg, pred_map, mask, gt_map)
    # the record itself: rows behind count are -1 / zeros, rows in front are the kept proposals in increasing index
    for i, n in enumerate(rec["count"]):
        want = [j for j in range(mask.shape[1]) if mask[i, j] and rec["obj_prob"][i, j] > cfg["conf_thresh"]]
        assert list(rec["index"][i, :n]) == want and (rec["index"][i, n:] == -1).all()
        assert not rec["corners8"][i, n:].any() and not rec["score"][i, n:].any() and not rec["cls"][i, n:].any()


@pytest.mark.parametrize("name", TQ.CASES)
def test_restated_quads_reproduce_the_reference(name):
    ep = TQ.case_inputs(name)
    rec = R.detect_quads(ep, loss_inputs.EVAL_CONFIG, "last_")
    pred_map, mask, corners = R.quads_to_lists(rec)
    _, _, _, gt_map, gt_corners = TQ.oracle_parse(ep, loss_inputs.EVAL_CONFIG)
    TQ.check_lists(name, pred_map, mask, corners, gt_map, gt_corners)
    for i in range(len(mask)):
        assert (rec["index"][i, rec["count"][i]:] == -1).all() and (rec["index_f1"][i, rec["count_f1"][i]:] == -1).all()
        assert not rec["verts4"][i, rec["count_f1"][i]:].any()


# ---------------------------------------------------------------------------------------------------------- mutants
def small_inputs(seed, B=2, K=12, nh=1, ns=3, ncls=4):
    rs = np.random.RandomState(seed)
    f32 = np.float32
    return dict(center=(rs.rand(B, K, 3) * 4).astype(f32), heading_scores=rs.randn(B, K, nh).astype(f32),
                heading_residuals=(0.1 * rs.randn(B, K, nh)).astype(f32), size_scores=rs.randn(B, K, ns).astype(f32),
                size_residuals=(0.05 * rs.randn(B, K, ns, 3)).astype(f32), sem_cls_scores=rs.randn(B, K, ncls).astype(f32),
                objectness_scores=rs.randn(B, K, 2).astype(f32), mean_size=0.4 + rs.rand(ns, 3))


def decode(inp, rule="zero", bev=False, mutant=None):
    return R.decode_boxes(inp["center"], inp["heading_scores"], inp["heading_residuals"], inp["size_scores"],
                          inp["size_residuals"], inp["sem_cls_scores"], inp["objectness_scores"], inp["mean_size"], rule,
                          bev=bev, mutant=mutant)


def test_mutant_last_maximum_fails_on_rows_with_exact_ties():
    inp = small_inputs(1)
    inp["sem_cls_scores"][0, 0] = [0.5, 2.0, 2.0, -1.0]               # the first maximum is 1, the last is 2
    inp["size_scores"][1, 3] = [7.0, 7.0, 7.0]
    good, bad = decode(inp), decode(inp, mutant="last_max")
    assert good["sem_cls"][0, 0] == 1 and good["size_cls"][1, 3] == 0
    assert bad["sem_cls"][0, 0] == 2 and bad["size_cls"][1, 3] == 2
    assert not np.array_equal(good["size"], bad["size"])                # the gathered residual row follows the class
    untied = small_inputs(1)
    assert np.array_equal(decode(untied)["sem_cls"], decode(untied, mutant="last_max")["sem_cls"])   # only ties tell


def test_argmax_of_rows_with_nan_is_the_first_nan():
    x = np.array([[0.0, np.nan, 5.0, 1.0], [3.0, np.nan, np.nan, 9.0], [np.nan, 1.0, 2.0, 3.0]], np.float32)
    assert list(R.argmax_first(x)) == [1, 1, 0]


def pack_case(seed=3, B=2, K=40):
    rs = np.random.RandomState(seed)
    keep = (rs.rand(B, K) < 0.6).astype(np.uint8)
    score = rs.rand(B, K).astype(np.float32)
    cls = rs.randint(0, 5, (B, K)).astype(np.int32)
    corners8 = rs.randn(B, K, 8, 3)
    sem_prob = rs.rand(B, K, 5).astype(np.float32)
    return keep, score, cls, corners8, sem_prob


def test_mutant_ge_threshold_fails_when_conf_is_a_probability_the_first_run_produced():
    keep, score, cls, corners8, sem_prob = pack_case()
    first = R.pack_boxes(keep, score, 0.3, cls, corners8, sem_prob)
    conf = float(first["score"][0, first["count"][0] // 2])             # a score the first run selected
    j = int(first["index"][0, first["count"][0] // 2])
    good = R.pack_boxes(keep, score, conf, cls, corners8, sem_prob)
    bad = R.pack_boxes(keep, score, conf, cls, corners8, sem_prob, mutant="ge_threshold")
    assert j not in good["index"][0] and j in bad["index"][0]
    assert bad["count"][0] == good["count"][0] + 1
    assert good["count"][0] == sum(1 for q in range(keep.shape[1]) if keep[0, q] and score[0, q] > np.float32(conf))


def test_mutant_score_order_fails_when_scores_do_not_fall_with_the_index():
    keep, score, cls, corners8, sem_prob = pack_case()
    good = R.pack_boxes(keep, score, 0.3, cls, corners8, sem_prob)
    bad = R.pack_boxes(keep, score, 0.3, cls, corners8, sem_prob, mutant="score_order")
    n = good["count"][0]
    assert n > 3 and np.array_equal(good["count"], bad["count"])
    assert (np.diff(good["index"][0, :n]) > 0).all()
    assert sorted(bad["index"][0, :n]) == list(good["index"][0, :n]) and not np.array_equal(good["index"], bad["index"])
    for name, a in (("cls", cls), ("score", score), ("corners8", corners8), ("sem_prob", sem_prob)):
        assert np.array_equal(good[name][0, :n], a[0, good["index"][0, :n]])        # the payload rides with its index


def test_mutant_tail_unwritten_fails_wherever_a_row_is_not_selected():
    keep, score, cls, corners8, sem_prob = pack_case()
    verts4 = np.random.RandomState(5).randn(*keep.shape, 4, 3).astype(np.float32)
    good = R.pack_quads(keep, score, 0.3, corners8, verts4)
    bad = R.pack_quads(keep, score, 0.3, corners8, verts4, mutant="tail_unwritten")
    for s in range(keep.shape[0]):
        n, m = good["count"][s], good["count_f1"][s]
        assert 0 < m <= n < keep.shape[1]
        assert (good["index"][s, n:] == -1).all() and not good["score"][s, n:].any() and not good["corners8"][s, n:].any()
        assert (good["index_f1"][s, m:] == -1).all() and not good["verts4"][s, m:].any()
        assert (bad["index"][s, n:] != -1).all() and np.isnan(bad["corners8"][s, n:]).all() and np.isnan(bad["verts4"][s, m:]).all()
        for name in ("index", "score", "corners8"):
            assert np.array_equal(good[name][s, :n], bad[name][s, :n])
    full = R.pack_quads(np.ones_like(keep), np.ones_like(score), 0.3, corners8, verts4, mutant="tail_unwritten")
    assert np.array_equal(full["corners8"], corners8)                    # nothing left over: the mutant cannot show


def test_mutant_bev_axis_fails_on_two_boxes_stacked_above_each_other():
    """two equal boxes, one 5 m above the other (depth-frame z = upright-camera -y): the bird's-eye view suppresses the
    weaker one, a flattening of the camera's z axis instead leaves their heights apart and keeps both"""
    inp = small_inputs(7, B=1, K=2)
    inp["center"][0] = [[1.0, 2.0, 0.5], [1.0, 2.0, 5.5]]
    inp["size_scores"][0] = [[3.0, 0.0, 0.0]] * 2
    inp["size_residuals"][:] = 0
    inp["objectness_scores"][0, :, 1] = [2.0, 1.0]
    from oracle import ap_oracle
    keeps = {}
    for mutant in (None, "bev_axis"):
        dec = decode(inp, bev=True, mutant=mutant)
        keeps[mutant] = ap_oracle.nms_3d(dec["aabb"][0], dec["obj_prob"][0], 0.25)
    assert list(keeps[None]) == [True, False] and list(keeps["bev_axis"]) == [True, True]
    good = decode(inp, bev=True)
    assert (good["aabb"][..., 1] == 0).all() and (good["aabb"][..., 4] == 1).all()
    assert np.array_equal(good["corners8"], decode(inp, bev=False)["corners8"])     # the corners are never flattened
    cfg = loss_inputs.eval_config(**TB.MODES["bev_old"])                # and the reference's own mode notices
    rec = R.detect_boxes(TB.inputs(), cfg, "last_", mutant="bev_axis")
    assert not np.array_equal(rec["keep"].astype(np.float64), TB.GOLD["bev_old.pred_mask"])


def test_bins_heading_folds_into_minus_pi_pi():
    inp = small_inputs(9, nh=12)
    inp["heading_scores"][0, 0] = -5
    inp["heading_scores"][0, 0, 11] = 5                                  # class 11: 11 * 30 deg > 180 deg
    dec = decode(inp, rule="bins")
    a = 11 * (2 * np.pi / 12) + np.float64(inp["heading_residuals"][0, 0, 11])
    assert dec["heading_cls"][0, 0] == 11 and dec["heading"][0, 0] == np.float32(a - 2 * np.pi)
    assert (np.abs(dec["heading"]) <= np.float32(np.pi)).all() and not (decode(inp)["heading"] != 0).any()


def test_probabilities_round_the_float64_value_once():
    inp = small_inputs(11, K=50, ncls=18)
    dec = decode(inp)
    assert dec["obj_prob"].dtype == np.float32 and dec["sem_prob64"].dtype == np.float64
    assert np.abs(dec["sem_prob64"].sum(-1) - 1).max() < 1e-14
    assert np.array_equal(dec["obj_prob"], dec["obj_prob64"].astype(np.float32))


def test_restated_corners_are_the_oracles_whoever_supplies_the_cosine():
    from oracle import ap_oracle
    rs = np.random.RandomState(0)
    c, s = (rs.rand(2, 9, 3) * 4).astype(np.float32), rs.rand(2, 9, 3) + 0.2
    h = ((rs.rand(2, 9) - 0.5) * 6).astype(np.float32)
    want = ap_oracle.box_corners(c, s, h)
    got = R.box_corners(c, s, h, (np.cos(h).astype(np.float32), np.sin(h).astype(np.float32)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(R.box_corners(c, s, h)[0], want[0])
