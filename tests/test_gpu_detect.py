"""GPU: the packed detections (csrc/detect.hip, models/ap_helper_pq.py: detect_predictions / detect_quad_predictions) against
the float64 restatement (tests/detect_restatement.py) element by element, against the existing parse functions on the same
device tensors, and under capture.

Bounds.  Class indices, size, heading, corners and every packed field are compared BIT FOR BIT.  The two probabilities are
evaluated in f64 and rounded to f32 once, so |p - p64| <= 2^-24 p + 1e-45 (half an ulp of a normal number is at most 2^-24 of
it; 1e-45 covers the subnormals).  Corners under the "bins" heading rule: they are f64 arithmetic on the f32 cosine and sine
of the f32 heading; the heading is compared bit for bit, and the restatement is handed the device's own cosf / sinf of it
(torch.cos / torch.sin on the device, compared bit for bit with the kernel's through the corners themselves), because which f32
a cosine routine returns for an angle is not the kernel's arithmetic.  With numpy's cosine the corners agree within BOX_TOL;
the test prints how many elements differ in the last bits.  Under rule "zero" the cosine is exactly 1 and nothing is handed over."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import capi
import detect_restatement as R
import loss_inputs
import test_parse_boxes as TB
import test_parse_quads as TQ

pytestmark = pytest.mark.gpu
NS, NCLS = 18, 18
CANARY = 0x5A
PAD = 256                                         # canary bytes behind every buffer


class Buf(object):
    """a device buffer of `shape` with PAD canary bytes behind it, pre-filled with 0xFF bytes (NaN for every float type)"""

    def __init__(self, shape, dtype, fill=0xFF):
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n + PAD,), fill, dtype=torch.uint8, device="cuda")
        self.raw[n:] = CANARY
        self.n = n
        self.t = self.raw[:n].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[self.n:] == CANARY).all())

    def numpy(self):
        return self.t.cpu().numpy()


def decode_inputs(seed, B, K, nh, ties=True):
    rs = np.random.RandomState(seed)
    f32 = np.float32
    inp = dict(center=(rs.rand(B, K, 3) * 4).astype(f32), heading_scores=rs.randn(B, K, nh).astype(f32),
               heading_residuals=(0.3 * rs.randn(B, K, nh)).astype(f32), size_scores=rs.randn(B, K, NS).astype(f32),
               size_residuals=(0.05 * rs.randn(B, K, NS, 3)).astype(f32), sem_cls_scores=(3 * rs.randn(B, K, NCLS)).astype(f32),
               objectness_scores=(4 * rs.randn(B, K, 2)).astype(f32), mean_size=0.4 + rs.rand(NS, 3))
    if ties:
        for j in range(0, K, 5):                  # exact ties at the maximum: the first wins
            row = inp["sem_cls_scores"][0, j]
            row[[3, 11, 17]] = row.max() + 1
            inp["size_scores"][0, j, [2, 9]] = 50.0
            if nh > 1:
                inp["heading_scores"][0, j, [nh - 1, 4]] = 60.0
    inp["objectness_scores"][0, 0] = [0.0, -120.0]                    # a probability far down (1e-52 in f64: 0 in f32)
    if K > 2:
        inp["objectness_scores"][0, 1] = [0.0, -95.0]                 # a subnormal f32
        inp["objectness_scores"][0, 2] = [0.0, 40.0]                  # 1 - 4e-18: rounds to 1
    return inp


def run_decode(inp, rule, bev=False, want_sem_prob=True):
    B, K, nh = inp["heading_scores"].shape
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    out = {"heading_cls": Buf((B, K), torch.int32), "size_cls": Buf((B, K), torch.int32), "sem_cls": Buf((B, K), torch.int32),
           "size": Buf((B, K, 3), torch.float64), "heading": Buf((B, K), torch.float32), "obj_prob": Buf((B, K), torch.float32),
           "sem_prob": Buf((B, K, NCLS), torch.float32), "corners8": Buf((B, K, 8, 3), torch.float64),
           "aabb": Buf((B, K, 6), torch.float64)}
    capi.ok("omnipq_decode_boxes", B, K, nh, NS, NCLS, capi.P(dev["center"]), capi.P(dev["heading_scores"]),
            capi.P(dev["heading_residuals"]), capi.P(dev["size_scores"]), capi.P(dev["size_residuals"]),
            capi.P(dev["sem_cls_scores"]), capi.P(dev["objectness_scores"]), capi.P(dev["mean_size"]),
            1 if rule == "bins" else 0, int(bev), *[capi.P(out[n].t) if (n != "sem_prob" or want_sem_prob) else capi.P(None)
                                                    for n in ("heading_cls", "size_cls", "sem_cls", "size", "heading", "obj_prob",
                                                              "sem_prob", "corners8", "aabb")])
    torch.cuda.synchronize()
    assert all(b.intact() for b in out.values())
    return {n: b.numpy() for n, b in out.items()}, dev


def device_trig(heading):
    h = torch.from_numpy(np.ascontiguousarray(heading)).cuda()
    return torch.cos(h).cpu().numpy(), torch.sin(h).cpu().numpy()


def within_one_rounding(p, p64):
    return np.abs(p.astype(np.float64) - p64) <= 2.0 ** -24 * p64 + 1e-45


@pytest.mark.parametrize("nh", [1, 12])
@pytest.mark.parametrize("B,K", [(1, 1), (2, 100), (3, 256), (1, 300), (1, 4096)])
def test_decode_against_the_float64_restatement_at_every_element(B, K, nh):
    rule = "zero" if nh == 1 else "bins"
    inp = decode_inputs(100 + K + nh, B, K, nh)
    got, _ = run_decode(inp, rule, bev=(K == 100))
    args = [inp[n] for n in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals",
                             "sem_cls_scores", "objectness_scores", "mean_size")]
    want = R.decode_boxes(*args, rule, bev=(K == 100), trig=device_trig if rule == "bins" else None)
    for n in ("heading_cls", "size_cls", "sem_cls"):
        assert np.array_equal(got[n], want[n]), n
    for n in ("size", "heading", "corners8", "aabb"):
        assert got[n].tobytes() == want[n].tobytes(), (n, int((got[n] != want[n]).sum()))
    host = R.decode_boxes(*args, rule, bev=(K == 100))
    print(f"B={B} K={K} nh={nh}: corner elements that differ from numpy's cosine: {int((got['corners8'] != host['corners8']).sum())}"
          f" of {got['corners8'].size}, max {np.abs(got['corners8'] - host['corners8']).max():.3g}")
    assert np.abs(got["corners8"] - host["corners8"]).max() <= TB.BOX_TOL
    if rule == "bins":
        assert (np.abs(got["heading"]) <= np.float32(np.pi)).all() and (got["heading"] != 0).any()
    for n in ("obj_prob", "sem_prob"):
        ok = within_one_rounding(got[n], want[n + "64"])
        print(f"  {n}: differs from the rounded f64 value at {int((got[n] != want[n]).sum())} of {got[n].size} elements")
        assert ok.all(), (n, got[n][~ok][:4], want[n + "64"][~ok][:4])
    if K > 2:
        assert got["obj_prob"][0, 0] == 0 and 0 < got["obj_prob"][0, 1] < 1.2e-38 and got["obj_prob"][0, 2] == 1


@pytest.mark.parametrize("rule", ["zero", "bins"])
def test_decode_and_box_corners_share_their_bits(rule):
    """omnipq_box_corners on the decoded centre, size and heading gives the decode's corners and extents bit for bit (one device
    function, csrc/box_geom.h), and both are the restatement's"""
    B, K, nh = 2, 257, (1 if rule == "zero" else 12)
    inp = decode_inputs(31, B, K, nh)
    got, dev = run_decode(inp, rule)
    size = torch.from_numpy(got["size"]).cuda()
    heading = torch.from_numpy(got["heading"]).cuda()
    corners, aabb = Buf((B, K, 8, 3), torch.float64), Buf((B, K, 6), torch.float64)
    capi.ok("omnipq_box_corners", ctypes.c_longlong(B * K), capi.P(dev["center"]), capi.P(size),
            capi.P(heading if rule == "bins" else None), capi.P(corners.t), capi.P(aabb.t))
    torch.cuda.synchronize()
    assert corners.intact() and aabb.intact()
    assert corners.numpy().tobytes() == got["corners8"].tobytes() and aabb.numpy().tobytes() == got["aabb"].tobytes()
    want = R.box_corners(inp["center"], got["size"], got["heading"], device_trig(got["heading"]) if rule == "bins" else None)
    assert corners.numpy().tobytes() == want[0].tobytes() and aabb.numpy().tobytes() == want[1].tobytes()


def test_decode_without_the_class_probabilities_leaves_their_buffer_alone():
    inp = decode_inputs(5, 2, 70, 1)
    got, _ = run_decode(inp, "zero", want_sem_prob=False)
    assert np.isnan(got["sem_prob"]).all()
    full, _ = run_decode(inp, "zero")
    for n in ("sem_cls", "size", "obj_prob", "corners8", "aabb"):
        assert got[n].tobytes() == full[n].tobytes()


def test_argmax_of_rows_with_nan_is_torch_argmax_on_the_device():
    """rows with one and with two NaNs, in front of, between and behind the largest number: whatever torch.argmax returns
    for the row on this device is the contract (torch is asked here, not remembered)"""
    inp = decode_inputs(9, 1, 64, 12, ties=False)
    nan = np.float32("nan")
    for j in range(0, 64):
        for name, n in (("heading_scores", 12), ("size_scores", NS), ("sem_cls_scores", NCLS)):
            row = inp[name][0, j]
            big = int(row.argmax())
            if j % 4 == 0:
                row[(big + 1 + j // 4) % n] = nan                       # one NaN, anywhere
            elif j % 4 == 1:
                row[(j // 4) % n] = nan
                row[(j // 4 + 1 + j // 8) % n] = nan                    # two NaNs
            elif j % 4 == 2:
                row[0] = nan                                            # in front
                row[n - 1] = nan                                        # and behind
    got, dev = run_decode(inp, "bins")
    seen = 0
    for name, out in (("heading_scores", "heading_cls"), ("size_scores", "size_cls"), ("sem_cls_scores", "sem_cls")):
        want = torch.argmax(dev[name], -1).cpu().numpy()
        seen += int(np.isnan(inp[name]).any(-1).sum())
        assert np.array_equal(got[out], want.astype(np.int32)), (name, np.flatnonzero(got[out] != want)[:5])
        assert np.array_equal(R.argmax_first(inp[name]), want.astype(np.int32))      # and the restatement says the same
    assert seen >= 3 * 40


# ------------------------------------------------------------------------------------------------------------- pack
def pack_inputs(seed, B, K, case):
    rs = np.random.RandomState(seed)
    score = rs.rand(B, K).astype(np.float32)
    if case == "none":
        keep = (rs.rand(B, K) < 0.5).astype(np.uint8)
        score[keep != 0] *= np.float32(0.29)                              # kept rows below the threshold, others above
    elif case == "all":
        keep = np.full((B, K), 3, np.uint8)                               # any non-zero byte counts
        score = (0.31 + 0.6 * score).astype(np.float32)
    elif case == "alternate":
        keep = np.zeros((B, K), np.uint8)
        keep[:, ::2] = 1
        score = (0.31 + 0.6 * score).astype(np.float32)
    else:
        keep = (rs.rand(B, K) < 0.6).astype(np.uint8)
        score[rs.rand(B, K) < 0.1] = np.float32(0.3)                      # exactly at the threshold: not selected
    cls = rs.randint(0, NCLS, (B, K)).astype(np.int32)
    corners8 = rs.randn(B, K, 8, 3)
    sem_prob = rs.rand(B, K, NCLS).astype(np.float32)
    verts4 = rs.randn(B, K, 4, 3).astype(np.float32)
    return keep, score, cls, corners8, sem_prob, verts4


def run_pack_boxes(keep, score, cls, corners8, sem_prob, conf=0.3):
    B, K = keep.shape
    dev = [torch.from_numpy(a).cuda() for a in (keep, score, cls, corners8)] + [None if sem_prob is None else torch.from_numpy(sem_prob).cuda()]
    out = {"count": Buf((B,), torch.int32), "index": Buf((B, K), torch.int32), "cls": Buf((B, K), torch.int32),
           "score": Buf((B, K), torch.float32), "corners8": Buf((B, K, 8, 3), torch.float64),
           "sem_prob": Buf((B, K, NCLS), torch.float32)}
    capi.ok("omnipq_pack_boxes", B, K, NCLS, capi.P(dev[0]), capi.P(dev[1]), ctypes.c_float(conf), capi.P(dev[2]),
            capi.P(dev[3]), capi.P(dev[4]), *[capi.P(out[n].t) for n in ("count", "index", "cls", "score", "corners8")],
            capi.P(out["sem_prob"].t if sem_prob is not None else None))
    torch.cuda.synchronize()
    assert all(b.intact() for b in out.values())
    return {n: b.numpy() for n, b in out.items()}


def run_pack_quads(keep, prob, corners8, verts4, conf=0.3, quad_thres=0.5):
    B, K = keep.shape
    dev = [torch.from_numpy(a).cuda() for a in (keep, prob, corners8, verts4)]
    out = {"count": Buf((B,), torch.int32), "index": Buf((B, K), torch.int32), "score": Buf((B, K), torch.float32),
           "corners8": Buf((B, K, 8, 3), torch.float64), "count_f1": Buf((B,), torch.int32),
           "index_f1": Buf((B, K), torch.int32), "verts4": Buf((B, K, 4, 3), torch.float32)}
    capi.ok("omnipq_pack_quads", B, K, capi.P(dev[0]), capi.P(dev[1]), ctypes.c_float(conf), ctypes.c_float(quad_thres),
            capi.P(dev[2]), capi.P(dev[3]), *[capi.P(out[n].t) for n in ("count", "index", "score", "corners8", "count_f1",
                                                                        "index_f1", "verts4")])
    torch.cuda.synchronize()
    assert all(b.intact() for b in out.values())
    return {n: b.numpy() for n, b in out.items()}


def same_bits(got, want, names):
    for n in names:
        assert got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes(), n


@pytest.mark.parametrize("case", ["none", "all", "alternate", "random"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 100, 257, 300, 1024, 4096])
def test_pack_against_the_restatement(K, B, case):
    keep, score, cls, corners8, sem_prob, verts4 = pack_inputs(7 * K + B, B, K, case)
    got = run_pack_boxes(keep, score, cls, corners8, sem_prob)
    want = R.pack_boxes(keep, score, 0.3, cls, corners8, sem_prob)
    names = ("count", "index", "cls", "score", "corners8", "sem_prob")
    same_bits(got, want, names)
    if case == "none":
        assert not got["count"].any()
    if case == "all":
        assert (got["count"] == K).all()
    if case == "alternate":
        assert (got["count"] == (K + 1) // 2).all()
    for s in range(B):
        n = got["count"][s]
        assert (got["index"][s, n:] == -1).all() and not got["cls"][s, n:].any()
        assert not got["corners8"][s, n:].view(np.uint8).any() and not got["sem_prob"][s, n:].view(np.uint8).any()
    assert not any(np.isnan(got[n]).any() for n in ("score", "corners8", "sem_prob"))        # the pre-fill was NaN
    same_bits(run_pack_boxes(keep, score, cls, corners8, sem_prob), got, names)                # two runs, the same bits
    bare = run_pack_boxes(keep, score, cls, corners8, None)                                    # without the class rows
    same_bits(bare, want, names[:-1])
    assert np.isnan(bare["sem_prob"]).all()

    gotq = run_pack_quads(keep, score, corners8, verts4)
    wantq = R.pack_quads(keep, score, 0.3, corners8, verts4)
    namesq = ("count", "index", "score", "corners8", "count_f1", "index_f1", "verts4")
    same_bits(gotq, wantq, namesq)
    for s in range(B):
        m = gotq["count_f1"][s]
        assert m <= gotq["count"][s] and (gotq["index_f1"][s, m:] == -1).all() and not gotq["verts4"][s, m:].view(np.uint8).any()
    assert not np.isnan(gotq["verts4"]).any() and not np.isnan(gotq["corners8"]).any()
    same_bits(run_pack_quads(keep, score, corners8, verts4), gotq, namesq)


def test_empty_batches_launch_nothing():
    null = capi.P(None)
    capi.ok("omnipq_pack_boxes", 0, 256, NCLS, *[null] * 2, ctypes.c_float(0.3), *[null] * 9)
    capi.ok("omnipq_pack_quads", 3, 0, *[null] * 2, ctypes.c_float(0.3), ctypes.c_float(0.5), *[null] * 9)
    capi.ok("omnipq_decode_boxes", 0, 0, 1, NS, NCLS, *[null] * 8, 0, 0, *[null] * 9)


# ------------------------------------------------------------------------------------------------------ end to end
class Bins(loss_inputs.EvalDatasetConfig):
    num_heading_bin = 12

    def class2angle(self, pred_cls, residual, to_label_format=True):
        a = pred_cls * (2 * np.pi / 12) + residual
        return a - 2 * np.pi if (to_label_format and a > np.pi) else a


END_TO_END = dict(TB.MODES, bins=dict(use_3d_nms=True, cls_nms=False, per_class_proposal=True, remove_empty_box=True,
                                      conf_thresh=0.3))
_FIXTURE = {}


def box_inputs(name):
    """the golden test's inputs; for "bins" with twelve heading classes drawn on top (computed once, never changed)"""
    if name not in _FIXTURE:
        ep = TB.inputs()
        if name == "bins":
            rs = np.random.RandomState(12)
            B, K = ep["last_center"].shape[:2]
            ep["last_heading_scores"] = rs.randn(B, K, 12).astype(np.float32)
            ep["last_heading_residuals"] = (0.2 * rs.randn(B, K, 12)).astype(np.float32)
        _FIXTURE[name] = ep
    return _FIXTURE[name]


def guard_inputs(ep, thresholds):
    """Guard the inputs, not the result: on the CPU, neighbouring objectness probabilities within a scene differ by more
    than 1e-6 relative (a few ulp of difference between two sigmoids cannot reorder the suppression) and every probability
    is further than 1e-5 from every threshold used."""
    p = 1.0 / (1.0 + np.exp(-ep["last_objectness_scores"][..., 1].astype(np.float64)))
    for row in p:
        srt = np.sort(row)
        assert ((srt[1:] - srt[:-1]) / srt[1:]).min() > 1e-6
    assert p.min() > 1e-30                                                 # conf_thresh = 0: every probability is above it
    for t in thresholds:
        if t > 0:
            assert np.abs(p - t).min() > 1e-5, t
    for name in ("last_size_scores", "last_sem_cls_scores"):
        srt = np.sort(ep[name].astype(np.float64), -1)
        assert (srt[..., -1] - srt[..., -2]).min() > 1e-4, name


@pytest.mark.parametrize("name", sorted(END_TO_END))
def test_detect_predictions_equal_parse_predictions_on_the_same_tensors(name):
    import ap_helper_pq
    cfg = loss_inputs.eval_config(**END_TO_END[name])
    if name == "bins":
        cfg["dataset_config"] = Bins()
    ep_np = box_inputs(name)
    guard_inputs(ep_np, {cfg["conf_thresh"]})
    ep = {k: torch.from_numpy(v).cuda() for k, v in ep_np.items()}
    want_map, want_mask = ap_helper_pq.parse_predictions(ep, cfg, "last_")
    det = ap_helper_pq.detect_predictions(ep, cfg, "last_")
    got_map, got_mask = det.to_host().to_lists()
    assert np.array_equal(got_mask, want_mask) and got_mask.dtype == want_mask.dtype
    assert [len(x) for x in got_map] == [len(x) for x in want_map] and sum(len(x) for x in got_map) > 20
    for g, w in zip(got_map, want_map):
        assert [p[0] for p in g] == [p[0] for p in w] and all(type(a[0]) is type(b[0]) for a, b in zip(g, w))
        assert all(a[1].tobytes() == b[1].tobytes() and a[1].shape == (8, 3) for a, b in zip(g, w))        # corners: the bits
        assert np.allclose([a[2] for a in g], [b[2] for b in w], rtol=2e-6, atol=1e-8)
        assert all(np.asarray(a[2]).dtype == np.float32 for a in g)
    if name in TB.MODES:                                                   # and the reference's own outputs
        TB.check(name, cfg, got_map, got_mask, ap_helper_pq.parse_groundtruths(ep, cfg))
        # the device record against the restatement: the structure exactly, the probabilities within their rounding
        want = R.detect_boxes(ep_np, cfg, "last_")
        for n in ("count", "index", "cls", "keep"):
            assert np.array_equal(getattr(det, n).cpu().numpy(), want[n]), n
        assert within_one_rounding(det.obj_prob.cpu().numpy(), want["decoded"]["obj_prob64"]).all()


@pytest.mark.parametrize("name", TQ.CASES)
def test_detect_quad_predictions_equal_parse_quad_predictions_bit_for_bit(name):
    import ap_helper_pq
    ep = {k: torch.from_numpy(v).cuda() for k, v in TQ.case_inputs(name).items()}
    want_map, want_mask, want_corners = ap_helper_pq.parse_quad_predictions(ep, loss_inputs.EVAL_CONFIG, "last_")
    got_map, got_mask, got_corners = ap_helper_pq.detect_quad_predictions(ep, loss_inputs.EVAL_CONFIG, "last_").to_lists()
    assert np.array_equal(got_mask, want_mask)
    assert [len(x) for x in got_map] == [len(x) for x in want_map] and [len(x) for x in got_corners] == [len(x) for x in want_corners]
    for g, w in zip(got_map, want_map):
        assert all(a[0] == 1 and a[1].tobytes() == b[1].tobytes() and np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes()
                   for a, b in zip(g, w))
    for g, w in zip(got_corners, want_corners):
        assert all(a.tobytes() == b.tobytes() and a.shape == (4, 3) for a, b in zip(g, w))
    assert sum(len(x) for x in got_corners) > 0


# --------------------------------------------------------------------------------------------- structure and capture
def test_every_field_is_a_view_of_the_record_and_out_allocates_nothing():
    import ap_helper_pq
    cfg = loss_inputs.eval_config(**TB.MODES["plain3d_empty"])
    cfgq = loss_inputs.EVAL_CONFIG
    ep = {k: torch.from_numpy(v).cuda() for k, v in TB.inputs().items()}
    epq = {k: torch.from_numpy(v).cuda() for k, v in TQ.case_inputs(TQ.CASES[0]).items()}
    det = ap_helper_pq.detect_predictions(ep, cfg, "last_")
    detq = ap_helper_pq.detect_quad_predictions(epq, cfgq, "last_")
    for d in (det, detq):
        assert d.record.dtype == torch.uint8 and d.record.is_contiguous() and d.record.dim() == 1
        base = d.record.untyped_storage().data_ptr()
        assert {"count", "index", "score", "corners8", "keep"} <= set(d.fields)
        for name, view in d.fields.items():
            assert view.untyped_storage().data_ptr() == base, name
            assert d.record.data_ptr() <= view.data_ptr() and \
                view.data_ptr() + view.numel() * view.element_size() <= d.record.data_ptr() + d.record.numel(), name
            assert getattr(d, name) is view
    first = det.record.clone(), detq.record.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = ap_helper_pq.detect_predictions(ep, cfg, "last_", out=det)
    againq = ap_helper_pq.detect_quad_predictions(epq, cfgq, "last_", out=detq)
    assert torch.cuda.memory_allocated() == before
    assert again is det and againq is detq
    assert torch.equal(det.record, first[0]) and torch.equal(detq.record, first[1])          # a pure function of the inputs
    with pytest.raises(ValueError, match="not a boxes record"):
        ap_helper_pq.detect_predictions(ep, cfg, "last_", out=detq)
    with pytest.raises(ValueError, match="not a boxes record"):
        ap_helper_pq.detect_predictions(ep, loss_inputs.eval_config(**TB.MODES["cls3d"]), "last_", out=det)   # other fields


def test_to_lists_asserts_a_pick_where_the_parse_function_does():
    import ap_helper_pq
    cfg = loss_inputs.eval_config(**TB.MODES["plain3d_empty"])
    ep = {k: torch.from_numpy(v).cuda() for k, v in TB.inputs().items()}
    ep["point_clouds"] = ep["point_clouds"] + 100.0                        # every box is empty: nothing can be picked
    det = ap_helper_pq.detect_predictions(ep, cfg, "last_")
    assert not det.keep.any() and not det.count.any() and (det.index == -1).all()
    with pytest.raises(AssertionError):
        det.to_lists()
    with pytest.raises(AssertionError):
        ap_helper_pq.parse_predictions(ep, cfg, "last_")


def test_layer_one_under_capture_replays_a_second_batch_bit_for_bit():
    """the object and the quad call with out= inside torch.cuda.graph, on one stream; the inputs are then overwritten with a
    second batch and the replay compared with eager calls on that batch"""
    import gc
    import ap_helper_pq
    cfg = loss_inputs.eval_config(**TB.MODES["plain3d_empty"])
    cfgq = loss_inputs.EVAL_CONFIG
    keys = [k for k in TB.inputs() if k.startswith("last_") or k == "point_clouds"]
    keysq = [k for k in TQ.case_inputs(TQ.CASES[0]) if k.startswith("last_")]
    first = {k: TB.inputs()[k] for k in keys}
    firstq = {k: TQ.case_inputs(TQ.CASES[0])[k] for k in keysq}
    second = {k: loss_inputs.make_eval_boxes(int(TB.GOLD["seed"][0]) + 1)[k] for k in keys}
    B, KQ = firstq["last_quad_scores"].shape[:2]
    secondq = {k: loss_inputs.make_eval(91, B=B, KQ=KQ, two_walls_scene=False)[k] for k in keysq}
    ep = {k: torch.from_numpy(v).cuda() for k, v in first.items()}
    epq = {k: torch.from_numpy(v).cuda() for k, v in firstq.items()}
    det = ap_helper_pq.detect_predictions(ep, cfg, "last_")
    detq = ap_helper_pq.detect_quad_predictions(epq, cfgq, "last_")
    torch.cuda.synchronize()
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ap_helper_pq.detect_predictions(ep, cfg, "last_", out=det)
        ap_helper_pq.detect_quad_predictions(epq, cfgq, "last_", out=detq)
    for k in keys:
        ep[k].copy_(torch.from_numpy(second[k]))
    for k in keysq:
        epq[k].copy_(torch.from_numpy(secondq[k]))
    for d in (det, detq):
        for name, view in d.fields.items():
            if name != "mean_size":                                        # an input of the decode, not a result
                view.view(torch.uint8).fill_(0xEE)
    graph.replay()
    torch.cuda.synchronize()
    eager = ap_helper_pq.detect_predictions({k: v.clone() for k, v in ep.items()}, cfg, "last_")
    eagerq = ap_helper_pq.detect_quad_predictions({k: v.clone() for k, v in epq.items()}, cfgq, "last_")
    assert torch.equal(det.record, eager.record) and torch.equal(detq.record, eagerq.record)
    assert int(det.count.sum()) > 0 and int(detq.count.sum()) > 0
    firstrun = ap_helper_pq.detect_predictions({k: torch.from_numpy(v).cuda() for k, v in first.items()}, cfg, "last_")
    assert not torch.equal(firstrun.record, det.record)                    # the second batch is another batch
    got = det.to_host().to_lists()
    want = ap_helper_pq.parse_predictions(ep, cfg, "last_")
    assert [len(x) for x in got[0]] == [len(x) for x in want[0]] and np.array_equal(got[1], want[1])
