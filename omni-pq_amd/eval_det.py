"""Detection metrics of the evaluation loop -- the reference's `utils/eval_det.py` / `utils/box_util.py` pieces that
`APCalculator` / `QUADAPCalculator.compute_metrics` need, host-side numpy as there:

    box3d_iou(corners1, corners2)            utils/box_util.py:93-118   (oriented boxes, up = -Y: footprint clipping x height)
    voc_ap(rec, prec, use_07_metric=False)   utils/eval_det.py:24-55
    eval_det_cls(pred, gt, ovthresh, ...)    utils/eval_det.py:75-161
    eval_det(pred_all, gt_all, ovthresh,...) utils/eval_det.py:168-208  (= eval_det_multiprocessing :211-256 without the
                                                                          process pool: a few hundred boxes per class)

The reference clips the two footprints with Sutherland-Hodgman and takes the area of the result from scipy's ConvexHull;
the clipped polygon of two convex quadrilaterals is convex, so its shoelace area is the same number and no hull is built.

Opt-in device route (csrc/eval_iou.hip), below the reference's functions, which it leaves untouched:

    box3d_iou_batch(corners_a, corners_b)    box3d_iou elementwise on device tensors
    pack_segments(pred_all, gt_all)          eval_det's grouping, flattened into (class, scan) segments; pure numpy
    match_from_best(conf, seg, ovmax, jmax, npos, ovthresh)     eval_det_cls's greedy pass from each detection's best overlap
    eval_det_device(pred_all, gt_all, ovthresh, ...)            eval_det with the overlaps from the kernel; several thresholds
                                                                from one pass
"""
import numpy as np


def _clip(subject, clip):
    """Sutherland-Hodgman: `subject` (list of (x, y)) clipped by the convex counter-clockwise polygon `clip`; [] if empty."""
    out = list(subject)
    a = clip[-1]
    for b in clip:
        if not out:
            return []
        src, out = out, []
        ex, ey = b[0] - a[0], b[1] - a[1]

        def inside(p):
            return ex * (p[1] - a[1]) > ey * (p[0] - a[0])

        s = src[-1]
        for e in src:
            e_in, s_in = inside(e), inside(s)
            if e_in != s_in:
                dcx, dcy = a[0] - b[0], a[1] - b[1]
                dpx, dpy = s[0] - e[0], s[1] - e[1]
                n1 = a[0] * b[1] - a[1] * b[0]
                n2 = s[0] * e[1] - s[1] * e[0]
                n3 = 1.0 / (dcx * dpy - dcy * dpx)
                out.append(((n1 * dpx - n2 * dcx) * n3, (n1 * dpy - n2 * dcy) * n3))
            if e_in:
                out.append(e)
            s = e
        a = b
    return out


def _shoelace(poly):
    p = np.asarray(poly, dtype=np.float64)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, 1)) - np.dot(y, np.roll(x, 1)))


def _volume(c):
    a = np.sqrt(((c[0] - c[1]) ** 2).sum())
    b = np.sqrt(((c[1] - c[2]) ** 2).sum())
    h = np.sqrt(((c[0] - c[4]) ** 2).sum())
    return a * b * h


def box3d_iou(corners1, corners2):
    """corners (8, 3) as get_3d_box lays them out (rows 0-3 the top face, 4-7 the bottom face, up = -Y) -> (iou3d, iou2d)."""
    c1, c2 = np.asarray(corners1, np.float64), np.asarray(corners2, np.float64)
    rect1 = [(c1[i, 0], c1[i, 2]) for i in range(3, -1, -1)]
    rect2 = [(c2[i, 0], c2[i, 2]) for i in range(3, -1, -1)]
    area1, area2 = _shoelace(rect1), _shoelace(rect2)
    inter = _clip(rect1, rect2)
    inter_area = _shoelace(inter) if len(inter) >= 3 else 0.0
    iou_2d = inter_area / (area1 + area2 - inter_area)
    ymax = min(c1[0, 1], c2[0, 1])
    ymin = max(c1[4, 1], c2[4, 1])
    inter_vol = inter_area * max(0.0, ymax - ymin)
    return inter_vol / (_volume(c1) + _volume(c2) - inter_vol), iou_2d


def get_iou_obb(bb1, bb2):
    return box3d_iou(bb1, bb2)[0]


def voc_ap(rec, prec, use_07_metric=False):
    if use_07_metric:                                   # 11-point interpolation
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            ap += (np.max(prec[rec >= t]) if np.sum(rec >= t) else 0.0) / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]      # precision envelope
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def eval_det_cls(pred, gt, ovthresh=0.25, use_07_metric=False, get_iou_func=get_iou_obb):
    """pred {img_id: [(bbox, score)]}, gt {img_id: [bbox]} -> (rec, prec, ap) for one class: detections by decreasing
    score, each matched to the ground truth of its image it overlaps most; a second match of the same box is a false
    positive."""
    npos = sum(len(v) for v in gt.values())
    taken = {img: [False] * len(boxes) for img, boxes in gt.items()}
    dets = [(img, box, score) for img, lst in pred.items() for box, score in lst]
    conf = np.array([d[2] for d in dets], dtype=np.float64)
    order = np.argsort(-conf)
    tp, fp = np.zeros(len(dets)), np.zeros(len(dets))
    for d, idx in enumerate(order):
        img, box, _ = dets[idx]
        boxes = gt.get(img, [])
        ovmax, jmax = -np.inf, -1
        for j, g in enumerate(boxes):
            iou = get_iou_func(np.asarray(box, float), np.asarray(g, float))
            if iou > ovmax:
                ovmax, jmax = iou, j
        if ovmax > ovthresh and not taken[img][jmax]:
            tp[d] = 1.0
            taken[img][jmax] = True
        else:
            fp[d] = 1.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def eval_det(pred_all, gt_all, ovthresh=0.25, use_07_metric=False, get_iou_func=get_iou_obb):
    """pred_all {img_id: [(classname, bbox, score)]}, gt_all {img_id: [(classname, bbox)]} -> ({class: rec}, {class: prec},
    {class: ap}); classes that only occur in the predictions count with an empty ground truth."""
    pred, gt = {}, {}
    for img, lst in pred_all.items():
        for cls, box, score in lst:
            pred.setdefault(cls, {}).setdefault(img, []).append((box, score))
            gt.setdefault(cls, {}).setdefault(img, [])
    for img, lst in gt_all.items():
        for cls, box in lst:
            gt.setdefault(cls, {}).setdefault(img, []).append(box)
    rec, prec, ap = {}, {}, {}
    for cls in gt:
        if cls in pred:
            rec[cls], prec[cls], ap[cls] = eval_det_cls(pred[cls], gt[cls], ovthresh, use_07_metric, get_iou_func)
        else:
            rec[cls], prec[cls], ap[cls] = 0, 0, 0
    return rec, prec, ap


eval_det_multiprocessing = eval_det


# ------------------------------------------------------------------------------------------------- the device route
# The overlaps of eval_det_cls's inner loop do not depend on the threshold and are data-parallel: csrc/eval_iou.hip computes,
# per detection, the best overlap with the ground truth of its (class, scan) segment and the index of the box that gave it
# (include/omnipq_eval.h: omnipq_obb_iou_best).  The greedy pass over the detections by decreasing score -- the only
# sequential part -- stays here, on the same `np.argsort(-conf)` of the same array.  Opt-in: eval_det() above is untouched.
def box3d_iou_batch(corners_a, corners_b):
    """(n, 8, 3) f64 device tensors -> (iou3d, iou2d) (n,) f64 device tensors: box3d_iou(corners_a[i], corners_b[i]) per i
    on the kernel (omnipq_obb_iou_pairs).  No CPU path: CPU tensors are refused."""
    import torch
    from pointnet2 import _ext
    for t, name in ((corners_a, "corners_a"), (corners_b, "corners_b")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"eval_det: `{name}` must be a GPU tensor (the HIP path has no CPU fallback)")
        if t.dtype != torch.float64 or t.dim() != 3 or tuple(t.shape[1:]) != (8, 3):
            raise ValueError(f"eval_det: `{name}` must be (n, 8, 3) float64")
    if corners_a.shape != corners_b.shape or corners_a.device != corners_b.device:
        raise ValueError("eval_det: corners_a and corners_b must have the same shape and device")
    a, b = corners_a.detach().contiguous(), corners_b.detach().contiguous()
    n = a.shape[0]
    iou3d = torch.empty(n, device=a.device, dtype=torch.float64)
    iou2d = torch.empty(n, device=a.device, dtype=torch.float64)
    _ext._run(_ext._lib.omnipq_obb_iou_pairs, a, n, _ext._ptr(a), _ext._ptr(b), _ext._ptr(iou3d), _ext._ptr(iou2d))
    return iou3d, iou2d


def pack_segments(pred_all, gt_all):
    """The inputs of eval_det() grouped as eval_det() groups them, flattened for omnipq_obb_iou_best.  Pure numpy.

    -> {"classes":   the classes in eval_det's order (the ground truth's insertion order; a class seen only in the
                     predictions is among them with an empty ground truth),
        "per_class": {class: None for a class without predictions (scored 0, 0, 0), else
                             {"lo", "hi": its detections are rows lo:hi of the flat arrays, in eval_det_cls's `dets` order,
                              "img": their scan ids, "conf": their scores as eval_det_cls builds them (f64),
                              "seg": their segment ids (= pred_seg[lo:hi]), "npos": the class's ground-truth count}},
        "pred8" (n_pred, 8, 3) f64, "pred_seg" (n_pred,) i32, "seg_start" (n_seg + 1,) i64, "gt8" (n_gt, 8, 3) f64}
    A segment is one (class, scan) pair that has predictions; its ground truth is gt8[seg_start[s]:seg_start[s + 1]]."""
    pred, gt = {}, {}
    for img, lst in pred_all.items():
        for cls, box, score in lst:
            pred.setdefault(cls, {}).setdefault(img, []).append((box, score))
            gt.setdefault(cls, {}).setdefault(img, [])
    for img, lst in gt_all.items():
        for cls, box in lst:
            gt.setdefault(cls, {}).setdefault(img, []).append(box)
    per_class, pred_boxes, gt_boxes, pred_seg, seg_start = {}, [], [], [], [0]
    for cls in gt:
        if cls not in pred:
            per_class[cls] = None
            continue
        lo = len(pred_boxes)
        dets = [(img, box, score) for img, lst in pred[cls].items() for box, score in lst]
        for img, lst in pred[cls].items():
            seg = len(seg_start) - 1
            gt_boxes.extend(gt[cls][img])
            seg_start.append(len(gt_boxes))
            pred_seg.extend([seg] * len(lst))
        pred_boxes.extend(d[1] for d in dets)
        per_class[cls] = {"lo": lo, "hi": len(pred_boxes), "img": [d[0] for d in dets],
                          "conf": np.array([d[2] for d in dets], dtype=np.float64),
                          "seg": np.asarray(pred_seg[lo:], dtype=np.int32),
                          "npos": sum(len(v) for v in gt[cls].values())}

    def boxes(lst):
        return np.ascontiguousarray(np.asarray(lst, dtype=np.float64).reshape(len(lst), 8, 3))

    return {"classes": list(gt), "per_class": per_class, "pred8": boxes(pred_boxes),
            "pred_seg": np.asarray(pred_seg, dtype=np.int32), "seg_start": np.asarray(seg_start, dtype=np.int64),
            "gt8": boxes(gt_boxes)}


def best_on_host(pack, get_iou_func=get_iou_obb):
    """(ovmax (n_pred,) f64, jmax (n_pred,) i32) of pack_segments()'s arrays by eval_det_cls's own loop: what
    omnipq_obb_iou_best computes, on the host."""
    n = len(pack["pred_seg"])
    ovmax, jmax = np.full(n, -np.inf), np.full(n, -1, dtype=np.int32)
    for i in range(n):
        j0, j1 = pack["seg_start"][pack["pred_seg"][i]:pack["pred_seg"][i] + 2]
        for j in range(j0, j1):
            iou = get_iou_func(pack["pred8"][i], pack["gt8"][j])
            if iou > ovmax[i]:
                ovmax[i], jmax[i] = iou, j - j0
    return ovmax, jmax


def best_on_device(pack, device=None, times=None):
    """The same pair from omnipq_obb_iou_best: ONE host-to-device copy of the packed arrays, one launch, one copy back.
    `times`, a dict, receives the wall seconds of "upload", "launch" and "download" (each ends in a synchronise)."""
    import ctypes
    import time
    import torch
    from pointnet2 import _ext
    n_pred, n_gt, n_seg = len(pack["pred_seg"]), len(pack["gt8"]), len(pack["seg_start"]) - 1
    if n_pred == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int32)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("eval_det: the device route needs a GPU (the HIP path has no CPU fallback)")
    clock = time.perf_counter
    t0 = clock()
    # 8-byte items first, so that every part starts aligned to its type
    parts = [pack["pred8"], pack["gt8"], pack["seg_start"], pack["pred_seg"]]
    host = np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts])
    buf = torch.from_numpy(host).to(device)
    offs = np.concatenate([[0], np.cumsum([p.nbytes for p in parts])])
    base = buf.data_ptr()
    out = torch.empty(n_pred * 12, device=device, dtype=torch.uint8)             # ovmax f64, then jmax i32
    if times is not None:
        torch.cuda.synchronize(device)
        t1 = clock()
    _ext._run(_ext._lib.omnipq_obb_iou_best, buf, n_pred, ctypes.c_void_p(base), ctypes.c_void_p(base + int(offs[3])),
              n_seg, ctypes.c_void_p(base + int(offs[2])), n_gt, ctypes.c_void_p(base + int(offs[1]) if n_gt else 0),
              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + n_pred * 8))
    if times is not None:
        torch.cuda.synchronize(device)
        t2 = clock()
    got = out.cpu().numpy()
    ovmax, jmax = got[:n_pred * 8].view(np.float64), got[n_pred * 8:].view(np.int32)
    if times is not None:
        times.update(upload=t1 - t0, launch=t2 - t1, download=clock() - t2)
    return ovmax, jmax


def match_from_best(conf, seg, ovmax, jmax, npos, ovthresh, use_07_metric=False):
    """(rec, prec, ap) of one class from each detection's best overlap: eval_det_cls's greedy pass without its loop.
    conf, seg, ovmax, jmax: per detection in `dets` order.  Visiting the detections by `np.argsort(-conf)` -- the call
    eval_det_cls makes, on the same array -- a detection is a true positive iff ovmax > ovthresh and no earlier one above
    the threshold chose the same ground-truth box (segment, jmax): a detection at or below the threshold takes nothing."""
    conf = np.asarray(conf, dtype=np.float64)
    order = np.argsort(-conf)
    above = np.asarray(ovmax)[order] > ovthresh
    jm = np.asarray(jmax, dtype=np.int64)[order] + 1                     # -1 (an empty segment) .. -> 0 ..
    key = np.asarray(seg, dtype=np.int64)[order] * (int(jm.max()) + 1 if len(jm) else 1) + jm
    cand = np.nonzero(above)[0]
    tp, fp = np.zeros(len(conf)), np.ones(len(conf))
    if len(cand):
        first = cand[np.unique(key[cand], return_index=True)[1]]         # the first in visiting order per chosen box
        tp[first], fp[first] = 1.0, 0.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def eval_from_best(pack, ovmax, jmax, ovthresh, use_07_metric=False):
    """eval_det's return triple for one threshold from pack_segments() and the per-detection best overlaps."""
    rec, prec, ap = {}, {}, {}
    for cls in pack["classes"]:
        c = pack["per_class"][cls]
        if c is None:
            rec[cls], prec[cls], ap[cls] = 0, 0, 0
        else:
            lo, hi = c["lo"], c["hi"]
            rec[cls], prec[cls], ap[cls] = match_from_best(c["conf"], c["seg"], ovmax[lo:hi], jmax[lo:hi], c["npos"],
                                                           ovthresh, use_07_metric)
    return rec, prec, ap


def eval_det_device(pred_all, gt_all, ovthresh=0.25, use_07_metric=False, get_iou_func=None, device=None):
    """eval_det() with the overlaps computed on the device: the same ({class: rec}, {class: prec}, {class: ap}).  `ovthresh`
    may be a sequence: then a list of such triples, one per threshold, from one upload, one launch and one download."""
    if get_iou_func is not None and get_iou_func is not get_iou_obb:
        raise ValueError("eval_det_device: the device computes get_iou_obb only; use eval_det() for another get_iou_func")
    pack = pack_segments(pred_all, gt_all)
    ovmax, jmax = best_on_device(pack, device)
    if np.ndim(ovthresh) == 0:
        return eval_from_best(pack, ovmax, jmax, ovthresh, use_07_metric)
    return [eval_from_best(pack, ovmax, jmax, t, use_07_metric) for t in ovthresh]
