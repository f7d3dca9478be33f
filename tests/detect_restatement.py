"""numpy / float64 restatement of the packed detections (include/omnipq_eval.h: omnipq_decode_boxes, omnipq_pack_boxes,
omnipq_pack_quads; models/ap_helper_pq.py: detect_predictions, detect_quad_predictions, Detections.to_lists) -- TEST
INFRASTRUCTURE ONLY.  The suppression, the quad decode and the points-in-box count are oracle/ap_oracle.py's.

Probabilities are returned in float64 (`obj_prob64`, `sem_prob64`: what the kernel rounds once) next to their float32
roundings; everything else carries the kernel's own types, so the GPU tests compare bits.

`mutant`: one of MUTANTS, a defect the tests must be able to see (tests/test_detect_restatement.py builds an input for each):
    last_max       the last maximum of a row instead of the first
    ge_threshold   `>= conf` instead of `> conf`
    score_order    selected rows in decreasing score instead of increasing index
    tail_unwritten rows behind count left as the pre-fill
    bev_axis       the bird's-eye-view flattening on the third axis instead of the second
"""
import numpy as np

from oracle import ap_oracle

MUTANTS = ("last_max", "ge_threshold", "score_order", "tail_unwritten", "bev_axis")
QUAD_THRES = 0.5
MAX_K = 4096
PREFILL = {"i": np.int32(-77), "f": np.nan}          # what "unwritten" looks like: the GPU tests pre-fill with NaN bytes


def argmax_first(x, mutant=None):
    """first maximum of the last axis; a NaN is larger than every number and the first NaN wins (np.argmax's rule too)"""
    x = np.asarray(x, np.float32)
    if mutant == "last_max":
        return (x.shape[-1] - 1 - np.argmax(x[..., ::-1], -1)).astype(np.int32)
    return np.argmax(x, -1).astype(np.int32)


def box_corners(center, size, heading, trig=None):
    """ap_oracle.box_corners, restated with the cosine and sine of the heading as an optional input: trig = (cos, sin), two
    f32 arrays.  The corners are f64 arithmetic on those two f32 numbers; WHICH f32 a cosine routine returns for an angle
    is the routine's business (numpy's and the device's may differ in the last bit), so a test that compares corners bit for
    bit hands over the device's own."""
    if trig is None:
        return ap_oracle.box_corners(center, size, heading)
    center, size = np.asarray(center, np.float32), np.asarray(size, np.float64)
    c, s = (np.asarray(t, np.float32).astype(np.float64)[..., None] for t in trig)
    cam = np.stack([center[..., 0], -center[..., 2], center[..., 1]], -1).astype(np.float64)
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1]) / 2.0
    sy = np.array([1, 1, 1, 1, -1, -1, -1, -1]) / 2.0
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1]) / 2.0
    x, y, z = size[..., 0:1] * sx, size[..., 2:3] * sy, size[..., 1:2] * sz
    corners = np.stack([c * x + s * z + cam[..., None, 0], y + cam[..., None, 1], -s * x + c * z + cam[..., None, 2]], -1)
    return corners, np.concatenate([corners.min(-2), corners.max(-2)], -1)


def decode_boxes(center, heading_scores, heading_residuals, size_scores, size_residuals, sem_cls_scores, objectness_scores,
                 mean_size, heading_rule, bev=False, mutant=None, trig=None):
    """-> dict: heading_cls / size_cls / sem_cls (B,K) i32, size (B,K,3) f64, heading (B,K) f32, obj_prob64 (B,K) f64 and
    obj_prob f32, sem_prob64 (B,K,ncls) f64 and sem_prob f32, corners8 (B,K,8,3) f64, aabb (B,K,6) f64.  heading_rule:
    "zero" | "bins".  trig: a function heading (B,K) f32 -> (cos, sin) f32 to take the place of numpy's (box_corners)."""
    f32, f64 = np.float32, np.float64
    center = np.asarray(center, f32)
    nh = np.asarray(heading_scores).shape[-1]
    out = {"heading_cls": argmax_first(heading_scores, mutant), "size_cls": argmax_first(size_scores, mutant),
           "sem_cls": argmax_first(sem_cls_scores, mutant)}
    hc, sc = out["heading_cls"].astype(np.int64), out["size_cls"].astype(np.int64)
    res = np.take_along_axis(np.asarray(size_residuals, f32), sc[..., None, None].repeat(3, -1), 2)[:, :, 0]
    out["size"] = np.asarray(mean_size, f64)[sc] + res.astype(f64)
    if heading_rule == "bins":
        hres = np.take_along_axis(np.asarray(heading_residuals, f32), hc[..., None], 2)[..., 0]
        per = 2 * np.pi / nh
        a = hc.astype(f64) * per + hres.astype(f64)
        out["heading"] = np.where(a > np.pi, a - 2 * np.pi, a).astype(f32)
    else:
        assert heading_rule == "zero"
        out["heading"] = np.zeros(center.shape[:2], f32)
    with np.errstate(over="ignore", invalid="ignore"):
        out["obj_prob64"] = 1.0 / (1.0 + np.exp(-np.asarray(objectness_scores, f32)[..., 1].astype(f64)))
        sem = np.asarray(sem_cls_scores, f32)
        e = np.exp(sem.astype(f64) - sem.max(-1, keepdims=True).astype(f64))
        total = np.zeros(e.shape[:-1], f64)
        for c in range(e.shape[-1]):                                     # in index order, as the kernel adds
            total = total + e[..., c]
        out["sem_prob64"] = e / total[..., None]
    out["obj_prob"] = out["obj_prob64"].astype(f32)
    out["sem_prob"] = out["sem_prob64"].astype(f32)
    out["corners8"], aabb = box_corners(center, out["size"], out["heading"], None if trig is None else trig(out["heading"]))
    if bev:
        axis = 2 if mutant == "bev_axis" else 1
        aabb = aabb.copy()
        aabb[..., axis], aabb[..., axis + 3] = 0.0, 1.0
    out["aabb"] = aabb
    return out


def _select(keep, score, conf, mutant):
    score = np.asarray(score, np.float32)
    hit = score >= np.float32(conf) if mutant == "ge_threshold" else score > np.float32(conf)
    sel = np.flatnonzero((np.asarray(keep) != 0) & hit)
    if mutant == "score_order":
        sel = sel[np.argsort(-score[sel], kind="stable")]
    return sel


def _pack(keep, score, conf, payload, mutant):
    """payload {name: (B,K,...) array}; -> count (B) i32, index (B,K) i32, {name: packed}"""
    B, K = np.asarray(keep).shape
    count = np.zeros(B, np.int32)
    tail = mutant == "tail_unwritten"
    index = np.full((B, K), PREFILL["i"] if tail else -1, np.int32)
    out = {n: (np.full(a.shape, PREFILL["i" if a.dtype.kind == "i" else "f"], a.dtype) if tail else np.zeros_like(a))
           for n, a in payload.items()}
    for s in range(B):
        sel = _select(keep[s], score[s], conf, mutant)
        count[s] = len(sel)
        index[s, :len(sel)] = sel
        for n, a in payload.items():
            out[n][s, :len(sel)] = a[s, sel]
    return count, index, out


def pack_boxes(keep, score, conf, cls, corners8, sem_prob=None, mutant=None):
    """-> dict count, index, cls, score, corners8 (, sem_prob): omnipq_pack_boxes"""
    assert np.asarray(keep).shape[1] <= MAX_K
    payload = {"cls": np.asarray(cls, np.int32), "score": np.asarray(score, np.float32), "corners8": np.asarray(corners8)}
    if sem_prob is not None:
        payload["sem_prob"] = np.asarray(sem_prob, np.float32)
    count, index, out = _pack(keep, score, conf, payload, mutant)
    return dict(out, count=count, index=index)


def pack_quads(keep, prob, conf, corners8, verts4, quad_thres=QUAD_THRES, mutant=None):
    """-> dict count, index, score, corners8 (the AP list), count_f1, index_f1, verts4 (the F1 list): omnipq_pack_quads"""
    assert np.asarray(keep).shape[1] <= MAX_K
    prob = np.asarray(prob, np.float32)
    count, index, ap = _pack(keep, prob, conf, {"score": prob, "corners8": np.asarray(corners8)}, mutant)
    count_f1, index_f1, f1 = _pack(keep, prob, quad_thres, {"verts4": np.asarray(verts4, np.float32)}, mutant)
    return dict(ap, count=count, index=index, count_f1=count_f1, index_f1=index_f1, verts4=f1["verts4"])


# ------------------------------------------------------------------------------------------------------ end to end
def heading_rule(dataset_config):
    """models/ap_helper_pq.py: _heading_rule, restated: what class2angle does to two probes"""
    nb = int(dataset_config.num_heading_bin)
    probe = [float(dataset_config.class2angle(np.int64(c), np.float32(r))) for c, r in ((0, 0.25), (max(nb - 1, 0), -0.1))]
    return "zero" if all(v == 0.0 for v in probe) else "bins"


def detect_boxes(ep, cfg, prefix="", mutant=None):
    """detect_predictions on numpy arrays -> record dict (decode + keep + pack), the probabilities rounded to f32 once"""
    DC = cfg["dataset_config"]
    rule = heading_rule(DC)
    dec = decode_boxes(ep[f"{prefix}center"], ep[f"{prefix}heading_scores"], ep[f"{prefix}heading_residuals"],
                       ep[f"{prefix}size_scores"], ep[f"{prefix}size_residuals"], ep[f"{prefix}sem_cls_scores"],
                       ep[f"{prefix}objectness_scores"], DC.mean_size_arr, rule, bev=not cfg["use_3d_nms"], mutant=mutant)
    B, K = dec["obj_prob"].shape
    head = dec["heading"] if rule == "bins" else None
    valid = None
    if cfg["remove_empty_box"]:
        valid = ap_oracle.points_in_boxes(np.asarray(ep["point_clouds"])[:, :, 0:3], ep[f"{prefix}center"], dec["size"], head)
    keep = np.zeros((B, K), np.uint8)
    for s in range(B):
        v = None if valid is None else valid[s]
        if cfg["use_3d_nms"] and cfg["cls_nms"]:
            keep[s] = ap_oracle.nms_3d_samecls(dec["aabb"][s], dec["obj_prob"][s], dec["sem_cls"][s], cfg["nms_iou"],
                                               cfg["use_old_type_nms"], v)
        else:                                            # plain 3D, or bird's-eye view on the extents decode flattened
            keep[s] = ap_oracle.nms_3d(dec["aabb"][s], dec["obj_prob"][s], cfg["nms_iou"], cfg["use_old_type_nms"], v)
    rec = pack_boxes(keep, dec["obj_prob"], cfg["conf_thresh"], dec["sem_cls"], dec["corners8"],
                     dec["sem_prob"] if cfg["per_class_proposal"] else None, mutant=mutant)
    rec.update(keep=keep, obj_prob=dec["obj_prob"], decoded=dec)
    return rec


def boxes_to_lists(rec, cfg):
    """Detections.to_lists() for objects: (batch_pred_map_cls, pred_mask) from the packed fields alone"""
    keep = rec["keep"].astype(bool)
    if cfg["use_3d_nms"] and not cfg["cls_nms"]:
        assert all(keep[i].any() for i in range(len(keep)))
    out = []
    for i, n in enumerate(rec["count"]):
        if cfg["per_class_proposal"]:
            out.append([(c, rec["corners8"][i, r], rec["sem_prob"][i, r, c] * rec["score"][i, r])
                        for c in range(cfg["dataset_config"].num_class) for r in range(n)])
        else:
            out.append([(int(rec["cls"][i, r]), rec["corners8"][i, r], rec["score"][i, r]) for r in range(n)])
    return out, keep.astype(np.float64)


def detect_quads(ep, cfg, prefix="", mutant=None):
    c8, aabb, verts = ap_oracle.decode_quads(ep[f"{prefix}quad_center"], ep[f"{prefix}normal_vector"], ep[f"{prefix}quad_size"])
    prob = ap_oracle.quad_prob(ep[f"{prefix}quad_scores"])
    thr = cfg["nms_iou_quad"] if "nms_iou_quad" in cfg else cfg["nms_iou"]
    keep = np.stack([ap_oracle.nms_3d(aabb[i], prob[i], thr, cfg["use_old_type_nms"]) for i in range(len(prob))]).astype(np.uint8)
    rec = pack_quads(keep, prob, cfg["conf_thresh"], c8, verts, mutant=mutant)
    rec.update(keep=keep, prob=prob)
    return rec


def quads_to_lists(rec):
    """Detections.to_lists() for quads: (batch_pred_map_cls, pred_mask, batch_pred_corners_list)"""
    keep = rec["keep"].astype(bool)
    assert all(keep[i].any() for i in range(len(keep)))
    pred = [[(1, rec["corners8"][i, r], rec["score"][i, r]) for r in range(n)] for i, n in enumerate(rec["count"])]
    corners = [[rec["verts4"][i, r] for r in range(n)] for i, n in enumerate(rec["count_f1"])]
    return pred, keep.astype(np.float64), corners
