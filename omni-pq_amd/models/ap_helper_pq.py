"""Evaluation-side consumer of the layout branch -- the reference's `models/ap_helper_pq.py` quad half on the kernels of
csrc/eval_ops.hip.  Same names, arguments and return values:

    parse_predictions(end_points, config_dict, prefix="")           ap_helper_pq.py:73-236
    parse_groundtruths(end_points, config_dict)                     :239-281
    APCalculator(ap_iou_thresh, class2type_map)                     :520-575   (step / compute_metrics / reset)
    parse_quad_predictions(end_points, config_dict, prefix="")      :323-460
    parse_quad_groundtruths(end_points, config_dict)                :462-517
    QUADAPCalculator(ap_iou_thresh, class2type_map, logger, logger_i)   :579-742   (step / compute_metrics / compute_F1 / reset)

The reference decodes every proposal in a Python loop with about ten `.detach().cpu().numpy()` reads each (B x 256 per
prediction head and batch, twice: a numpy and a tensor variant) and runs the suppression in numpy.  Here one launch decodes
all proposals (omnipq_parse_quads), one launch suppresses per scene (omnipq_nms3d), and the results come back in ONE
device-to-host copy; only the ragged Python lists the calculators consume are assembled on the host, as they must be.
QUADAPCalculator keeps the reference's host bookkeeping (lists of 4 x 3 corner arrays per scan) as its default route; its F1,
the number an evaluation epoch returns, can also be counted on the device (csrc/layout_f1.hip): LayoutF1 scores a
quad record against the batch's labels where both already are and is read once per epoch, and QUADAPCalculator(f1="device")
sends the accumulated lists through the same kernel.
There is no CPU path for the parsing: CPU tensors are refused (oracle/ap_oracle.py is the tests' CPU twin).
Both calculators take `iou="device"` (default "host", the reference's route): compute_metrics then gets the box overlaps from
csrc/eval_iou.hip through eval_det.eval_det_device, and compute_metrics_at(calculator, thresholds) scores several IoU thresholds
from one pass.
detect_predictions / detect_quad_predictions leave the same results ON THE DEVICE in one fixed-shape record (Detections) without
a host read, so they can sit in a captured graph (inference.CapturedInference); the two parse functions are unchanged.
"""
import ctypes

import numpy as np
import torch

import eval_det
from pointnet2 import _ext

_lib = _ext._lib

MAX_NUM_QUAD = 32
LENGTH = 0.1            # thickness given to a quad when it is boxed for NMS / AP
QUAD_THRES = 0.5        # probability above which a kept quad enters the F1 corner list
SAME_THRES = 0.40       # two corners closer than this are the same corner


def _f32(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"ap_helper_pq: `{name}` must be a GPU tensor (the HIP path has no CPU fallback)")
    return t.detach().float().contiguous()


def _decode(center, normal, size, scores=None, nms=None):
    """-> dict of device tensors: corners8 (B,K,8,3) f64, aabb (B,K,6) f64, verts4 (B,K,4,3) f32, prob (B,K) f32 and, with
    nms = (threshold, old_type), keep (B,K) u8."""
    c, n, s = _f32(center, "quad_center"), _f32(normal, "normal_vector"), _f32(size, "quad_size")
    B, K, _ = c.shape
    if n.shape != c.shape or tuple(s.shape) != (B, K, 2):
        raise ValueError("ap_helper_pq: quad_center / normal_vector must be (B, K, 3) and quad_size (B, K, 2)")
    dev = c.device
    out = {"corners8": torch.empty((B, K, 8, 3), device=dev, dtype=torch.float64),
           "aabb": torch.empty((B, K, 6), device=dev, dtype=torch.float64),
           "verts4": torch.empty((B, K, 4, 3), device=dev, dtype=torch.float32)}
    sc = None
    if scores is not None:
        sc = _f32(scores, "quad_scores")
        out["prob"] = torch.empty((B, K), device=dev, dtype=torch.float32)
    null = ctypes.c_void_p(0)
    _ext._run(_lib.omnipq_parse_quads, c, B, K, _ext._ptr(c), _ext._ptr(n), _ext._ptr(s),
              null if sc is None else _ext._ptr(sc), LENGTH, _ext._ptr(out["corners8"]),
              _ext._ptr(out["aabb"]), _ext._ptr(out["verts4"]), null if sc is None else _ext._ptr(out["prob"]))
    if nms is not None:
        out["keep"] = torch.empty((B, K), device=dev, dtype=torch.uint8)
        _ext._run(_lib.omnipq_nms3d, c, B, K, _ext._ptr(out["aabb"]), _ext._ptr(out["prob"]), null,
                  float(nms[0]), int(bool(nms[1])), _ext._ptr(out["keep"]))
    return out


def parse_quad_predictions(end_points, config_dict, prefix=""):
    """ Parse quad predictions to thin oriented boxes and suppress overlapping ones

    Args:
        end_points: dict
            {quad_center, normal_vector, quad_size, quad_scores} under `prefix`
        config_dict: dict
            {nms_iou (or nms_iou_quad), use_old_type_nms, conf_thresh}

    Returns:
        batch_pred_map_cls: a list of len == batch size (BS)
            [pred_list_i], i = 0, 1, ..., BS-1
            where pred_list_i = [(1, box corners (8,3) in the upright-camera frame, quad probability)_j]
            for the quads that survive NMS with probability > conf_thresh
        pred_mask: (BS, K) numpy array, 1 for the quads NMS kept
        batch_pred_corners_list: per sample the (4,3) corner arrays of the kept quads with probability > QUAD_THRES
    """
    scores = end_points[f'{prefix}quad_scores']
    thr = config_dict['nms_iou_quad'] if 'nms_iou_quad' in config_dict else config_dict['nms_iou']
    dec = _decode(end_points[f'{prefix}quad_center'], end_points[f'{prefix}normal_vector'], end_points[f'{prefix}quad_size'],
                  scores, nms=(thr, config_dict['use_old_type_nms']))
    B, K = dec["prob"].shape
    # one transfer for everything the lists are built from
    corners8 = dec["corners8"].cpu().numpy()
    verts4, prob, keep = dec["verts4"].cpu().numpy(), dec["prob"].cpu().numpy(), dec["keep"].cpu().numpy()
    assert all(keep[i].any() for i in range(B))                          # the reference asserts len(pick) > 0 (:425)
    pred_mask = keep.astype(np.float64)
    conf = config_dict['conf_thresh']
    batch_pred_map_cls = [[(1, corners8[i, j], prob[i, j]) for j in range(K) if keep[i, j] and prob[i, j] > conf]
                          for i in range(B)]
    batch_pred_corners_list = [[verts4[i, j] for j in range(K) if keep[i, j] and prob[i, j] > QUAD_THRES]
                               for i in range(B)]

    # the tensor twins the reference leaves in end_points (:446-455): f32 corners, sigmoid of the two logits
    corners_t = dec["corners8"].float().cpu()
    verts_t = dec["verts4"]
    prob_t = torch.sigmoid(scores.detach().float())
    end_points[f"{prefix}batch_pred_map_cls_tensor"] = [
        [(1, corners_t[i, j], prob_t[i, j]) for j in range(K) if keep[i, j] and prob[i, j] > conf] for i in range(B)]
    end_points[f"{prefix}batch_pred_corners_list_tensor"] = [
        [verts_t[i, j] for j in range(K) if keep[i, j] and prob[i, j] > 0.5] for i in range(B)]
    return batch_pred_map_cls, pred_mask, batch_pred_corners_list


def parse_quad_groundtruths(end_points, config_dict):
    """ Parse ground-truth quads to thin oriented boxes.

    Returns:
        batch_gt_map_cls: per sample [(1, box corners (8,3))_j] for j < num_gt_quads
        batch_gt_corners_list: per sample the (4,3) corner arrays for j < num_total_quads
    """
    center = end_points['gt_quad_centers'][:, :MAX_NUM_QUAD, 0:3]
    dec = _decode(center, end_points['gt_normal_vectors'][:, :MAX_NUM_QUAD], end_points['gt_quad_sizes'][:, :MAX_NUM_QUAD])
    corners8, verts4 = dec["corners8"].cpu().numpy(), dec["verts4"].cpu().numpy()
    B, K2 = corners8.shape[:2]
    # the data loader ships both counts once per quad proposal, (B, NUM_QUAD_PROPOSAL) (scannet_detection_dataset.py:301-304)
    n_gt = end_points['num_gt_quads'].detach().cpu().numpy().reshape(B, -1)
    n_total = end_points['num_total_quads'].detach().cpu().numpy().reshape(B, -1)
    col = lambda a, j: a[:, min(j, a.shape[1] - 1)]                      # noqa: E731
    batch_gt_map_cls = [[(1, corners8[i, j]) for j in range(K2) if j < col(n_gt, j)[i]] for i in range(B)]
    batch_gt_corners_list = [[verts4[i, j] for j in range(K2) if j < col(n_total, j)[i]] for i in range(B)]
    end_points['batch_gt_map_cls'] = batch_gt_map_cls
    return batch_gt_map_cls, batch_gt_corners_list


# ------------------------------------------------------------------------------------------------------- object boxes
def _heading_rule(dataset_config):
    """How the dataset config turns (heading class, residual) into an angle: ScanNet's returns 0 for everything (axis-aligned
    boxes, scannet/model_util_scannet.py:49-53), SUN RGB-D style configs return class * 2 pi / N + residual folded into
    (-pi, pi].  Probed once per config object; anything else is refused rather than guessed."""
    rule = getattr(dataset_config, "_omnipq_heading_rule", None)
    if rule is None:
        nb = int(dataset_config.num_heading_bin)
        probe = [float(dataset_config.class2angle(np.int64(c), np.float32(r))) for c, r in ((0, 0.25), (max(nb - 1, 0), -0.1))]
        if all(v == 0.0 for v in probe):
            rule = "zero"
        else:
            per = 2 * np.pi / nb
            want = []
            for c, r in ((0, 0.25), (max(nb - 1, 0), -0.1)):
                a = c * per + r
                want.append(a - 2 * np.pi if a > np.pi else a)
            if np.allclose(probe, want, atol=1e-6):
                rule = "bins"
            else:
                raise NotImplementedError("ap_helper_pq: unknown class2angle convention of the dataset config")
        try:
            dataset_config._omnipq_heading_rule = rule
        except Exception:
            pass
    return rule


def _box_params(center, heading_cls, heading_res, size_cls, size_res, dataset_config):
    """(B,K,.) device tensors -> center f32 (B,K,3), size f64 (B,K,3) = class2size, heading f32 (B,K) | None."""
    means = torch.from_numpy(np.asarray(dataset_config.mean_size_arr, dtype=np.float64)).to(center.device)
    size = means[size_cls] + size_res.double()
    heading = None
    if _heading_rule(dataset_config) == "bins":
        per = 2 * np.pi / int(dataset_config.num_heading_bin)
        ang = heading_cls.double() * per + heading_res.double()
        heading = torch.where(ang > np.pi, ang - 2 * np.pi, ang).float().contiguous()
    return center.detach().float().contiguous(), size.contiguous(), heading


def _corners(center, size, heading):
    B, K, _ = center.shape
    corners8 = torch.empty((B, K, 8, 3), device=center.device, dtype=torch.float64)
    aabb = torch.empty((B, K, 6), device=center.device, dtype=torch.float64)
    null = ctypes.c_void_p(0)
    _ext._run(_lib.omnipq_box_corners, center, B * K, _ext._ptr(center), _ext._ptr(size),
              null if heading is None else _ext._ptr(heading), _ext._ptr(corners8), _ext._ptr(aabb))
    return corners8, aabb


def parse_predictions(end_points, config_dict, prefix=""):
    """ Parse predictions to OBB parameters and suppress overlapping boxes

    Args:
        end_points: dict
            {point_clouds, center, heading_scores, heading_residuals,
            size_scores, size_residuals, sem_cls_scores, objectness_scores} under `prefix`
        config_dict: dict
            {dataset_config, remove_empty_box, use_3d_nms, nms_iou,
            use_old_type_nms, cls_nms, conf_thresh, per_class_proposal}

    Returns:
        batch_pred_map_cls: a list of len == batch size (BS)
            [pred_list_i], i = 0, 1, ..., BS-1
            where pred_list_i = [(pred_sem_cls, box corners (8,3), box_score)_j]
        pred_mask: (BS, K) numpy array, 1 for the boxes NMS kept
    """
    DC = config_dict['dataset_config']
    center = _f32(end_points[f'{prefix}center'], 'center')
    heading_cls = torch.argmax(end_points[f'{prefix}heading_scores'], -1)
    heading_res = torch.gather(end_points[f'{prefix}heading_residuals'].detach(), 2, heading_cls.unsqueeze(-1)).squeeze(2)
    size_cls = torch.argmax(end_points[f'{prefix}size_scores'], -1)
    size_res = torch.gather(end_points[f'{prefix}size_residuals'].detach(), 2,
                            size_cls[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
    sem_scores = end_points[f'{prefix}sem_cls_scores'].detach().float()
    pred_sem_cls = torch.argmax(sem_scores, -1)
    center, size, heading = _box_params(center, heading_cls, heading_res, size_cls, size_res, DC)
    corners8_t, aabb = _corners(center, size, heading)
    B, K = center.shape[:2]
    dev = center.device
    null = ctypes.c_void_p(0)

    valid = None
    if config_dict['remove_empty_box']:
        pc = _f32(end_points['point_clouds'][:, :, 0:3], 'point_clouds')
        valid = torch.empty((B, K), device=dev, dtype=torch.uint8)
        _ext._run(_lib.omnipq_points_in_boxes, pc, B, pc.shape[1], K, _ext._ptr(pc), _ext._ptr(center), _ext._ptr(size),
                  null if heading is None else _ext._ptr(heading), 5, _ext._ptr(valid))
    obj_prob_t = torch.sigmoid(end_points[f'{prefix}objectness_scores'].detach().float())[:, :, 1].contiguous()
    keep = torch.empty((B, K), device=dev, dtype=torch.uint8)
    vptr = null if valid is None else _ext._ptr(valid)
    thr, old = float(config_dict['nms_iou']), int(bool(config_dict['use_old_type_nms']))
    if not config_dict['use_3d_nms']:
        # bird's-eye-view suppression on (x, z) extents: the 3D kernel with a unit second axis
        flat = aabb.clone()
        flat[..., 1] = 0.0
        flat[..., 4] = 1.0
        _ext._run(_lib.omnipq_nms3d, center, B, K, _ext._ptr(flat), _ext._ptr(obj_prob_t), vptr, thr, old, _ext._ptr(keep))
    elif not config_dict['cls_nms']:
        _ext._run(_lib.omnipq_nms3d, center, B, K, _ext._ptr(aabb), _ext._ptr(obj_prob_t), vptr, thr, old, _ext._ptr(keep))
    else:
        cls32 = pred_sem_cls.int().contiguous()
        _ext._run(_lib.omnipq_nms3d_samecls, center, B, K, _ext._ptr(aabb), _ext._ptr(obj_prob_t), vptr, _ext._ptr(cls32),
                  thr, old, _ext._ptr(keep))

    # one transfer per array; the ragged lists are host data by nature
    corners8 = corners8_t.cpu().numpy()
    keep_h = keep.cpu().numpy().astype(bool)
    obj_prob = obj_prob_t.cpu().numpy()
    sem_probs = torch.softmax(sem_scores, -1).cpu().numpy()
    sem_cls_h = pred_sem_cls.cpu().numpy()
    if config_dict['use_3d_nms'] and not config_dict['cls_nms']:
        assert all(keep_h[i].any() for i in range(B))                     # the reference asserts len(pick) > 0 here only
    pred_mask = keep_h.astype(np.float64)
    conf = config_dict['conf_thresh']
    batch_pred_map_cls = []
    for i in range(B):
        sel = [j for j in range(K) if keep_h[i, j] and obj_prob[i, j] > conf]
        if config_dict['per_class_proposal']:
            batch_pred_map_cls.append([(ii, corners8[i, j], sem_probs[i, j, ii] * obj_prob[i, j])
                                       for ii in range(DC.num_class) for j in sel])
        else:
            batch_pred_map_cls.append([(int(sem_cls_h[i, j]), corners8[i, j], obj_prob[i, j]) for j in sel])
    return batch_pred_map_cls, pred_mask


def parse_groundtruths(end_points, config_dict):
    """ Parse groundtruth labels to OBB parameters.

    Returns:
        batch_gt_map_cls: a list of len == batch_size (BS) of [(gt_sem_cls, box corners (8,3))_j] over the boxes whose
        box_label_mask is 1
    """
    DC = config_dict['dataset_config']
    center = _f32(end_points['center_label'][:, :, 0:3], 'center_label')
    center, size, heading = _box_params(center, end_points['heading_class_label'].long(),
                                        end_points['heading_residual_label'].float(),
                                        end_points['size_class_label'].long(), end_points['size_residual_label'].float(), DC)
    corners8 = _corners(center, size, heading)[0].cpu().numpy()
    mask = end_points['box_label_mask'].detach().cpu().numpy()
    sem = end_points['sem_cls_label'].detach().cpu().numpy()
    B, K2 = mask.shape
    batch_gt_map_cls = [[(int(sem[i, j]), corners8[i, j]) for j in range(K2) if mask[i, j] == 1] for i in range(B)]
    end_points['batch_gt_map_cls'] = batch_gt_map_cls
    return batch_gt_map_cls


# ------------------------------------------------------------------------------------------------- packed detections
# The same results as the two parse functions above, left ON THE DEVICE in one fixed-shape record: decode,
# (points in boxes,) suppression and a stable compaction, four launches at most for the objects and three for the quads,
# no host read and -- with `out=` -- no allocation, so the calls can sit in a captured graph (inference.CapturedInference).
MAX_DECODE_CLASSES = int(_lib.omnipq_decode_boxes_max_classes())        # nh, ns, ncls: the library's own limit
MAX_PROPOSALS = 4096                                                    # k: the suppression kernel's limit

_I32, _F32, _F64, _U8 = torch.int32, torch.float32, torch.float64, torch.uint8
_NUMPY = {_I32: np.dtype(np.int32), _F32: np.dtype(np.float32), _F64: np.dtype(np.float64), _U8: np.dtype(np.uint8)}


def detections_layout(kind, B, K, ncls=0, ns=0, per_class=False):
    """-> ([(name, dtype, shape, byte offset)], result bytes, total bytes) of a record.  Pure.  The RESULT fields, what
    to_lists() reads, come first and are what to_host() copies; the decode's intermediates follow.  Every offset is a multiple
    of 16."""
    if kind == "boxes":
        result = [("count", _I32, (B,)), ("index", _I32, (B, K)), ("cls", _I32, (B, K)), ("score", _F32, (B, K)),
                  ("corners8", _F64, (B, K, 8, 3)), ("keep", _U8, (B, K))]
        if per_class:
            result.append(("sem_prob", _F32, (B, K, ncls)))
        rest = [("obj_prob", _F32, (B, K)), ("heading_cls", _I32, (B, K)), ("size_cls", _I32, (B, K)),
                ("sem_cls", _I32, (B, K)), ("size", _F64, (B, K, 3)), ("heading", _F32, (B, K)),
                ("all_corners8", _F64, (B, K, 8, 3)), ("aabb", _F64, (B, K, 6)), ("valid", _U8, (B, K)),
                ("mean_size", _F64, (ns, 3))]
        if per_class:
            rest.append(("all_sem_prob", _F32, (B, K, ncls)))
    elif kind == "quads":
        result = [("count", _I32, (B,)), ("index", _I32, (B, K)), ("score", _F32, (B, K)), ("corners8", _F64, (B, K, 8, 3)),
                  ("count_f1", _I32, (B,)), ("index_f1", _I32, (B, K)), ("verts4", _F32, (B, K, 4, 3)), ("keep", _U8, (B, K))]
        rest = [("prob", _F32, (B, K)), ("all_corners8", _F64, (B, K, 8, 3)), ("aabb", _F64, (B, K, 6)),
                ("all_verts4", _F32, (B, K, 4, 3))]
    else:
        raise ValueError(f"ap_helper_pq: a record is of kind 'boxes' or 'quads', not {kind!r}")
    fields, off, result_bytes = [], 0, 0
    for i, (name, dtype, shape) in enumerate(result + rest):
        fields.append((name, dtype, tuple(shape), off))
        off += -(-int(np.prod(shape, dtype=np.int64)) * _NUMPY[dtype].itemsize // 16) * 16
        if i == len(result) - 1:
            result_bytes = off
    return fields, result_bytes, off


class Detections(object):
    """The detections of a batch on the device.  `record` is ONE contiguous uint8 tensor; every field is a typed view into
    it (attributes, and `fields` by name): count (B) i32, then per scene rows [0, count) of index / cls / score / corners8
    (/ sem_prob) in increasing proposal index -- rows behind count hold index -1 and zeros -- keep (B,K) u8, and the
    decode's intermediates (obj_prob, size, heading, aabb, ...).  A record is a pure function of the inputs it was computed
    from.  Made by detect_predictions / detect_quad_predictions; hand it back as `out=` to have it rewritten in place."""

    def __init__(self, kind, B, K, device, ncls=0, ns=0, per_class=False, meta=None):
        self.kind, self.B, self.K, self.ncls, self.ns, self.per_class = kind, B, K, ncls, ns, per_class
        self.layout, self.result_bytes, nbytes = detections_layout(kind, B, K, ncls, ns, per_class)
        self.record = torch.zeros((max(nbytes, 16),), device=device, dtype=torch.uint8)
        self.fields = _views(self.record, self.layout)
        self.meta = dict(meta or {})                 # host-side constants to_lists() needs (asserting mode, class count)
        self._host = self._event = None

    def __getattr__(self, name):
        fields = self.__dict__.get("fields")
        if fields is not None and name in fields:
            return fields[name]
        raise AttributeError(name)

    def matches(self, kind, B, K, device, ncls=0, ns=0, per_class=False):
        return (self.kind, self.B, self.K, self.ncls, self.ns, self.per_class, self.record.device) == \
            (kind, B, K, ncls, ns, per_class, device)

    def to_host(self):
        """Copies the record's result fields into a pinned twin with ONE non-blocking copy on the current stream and records
        an event behind it.  Returns self."""
        if self._host is None:
            self._host = torch.empty((self.record.numel(),), dtype=torch.uint8, pin_memory=True)
            self._event = torch.cuda.Event()
        n = self.result_bytes
        self._host[:n].copy_(self.record[:n], non_blocking=True)
        self._event.record()
        return self

    def host_fields(self):
        """{name: numpy copy} of the result fields as the last to_host() left them; waits on its event."""
        if self._event is None:
            self.to_host()
        self._event.synchronize()
        flat = self._host.numpy()
        out = {}
        for name, dtype, shape, off in self.layout:
            if off >= self.result_bytes:
                break
            a = _NUMPY[dtype]
            n = int(np.prod(shape, dtype=np.int64))
            out[name] = flat[off:off + n * a.itemsize].view(a).reshape(shape).copy()
        return out

    def to_lists(self):
        """What the parse function of this record's kind returns, built from the pinned twin alone:
        (batch_pred_map_cls, pred_mask) for objects, (batch_pred_map_cls, pred_mask, batch_pred_corners_list) for quads.
        Asserts a non-empty pick per scene where the parse function does."""
        h = self.host_fields()
        keep = h["keep"].astype(bool)
        if self.meta.get("assert_pick", False):
            assert all(keep[i].any() for i in range(self.B))
        pred_mask = keep.astype(np.float64)
        corners8, score, count = h["corners8"], h["score"], h["count"]
        if self.kind == "quads":
            pred = [[(1, corners8[i, r], score[i, r]) for r in range(count[i])] for i in range(self.B)]
            return pred, pred_mask, [[h["verts4"][i, r] for r in range(h["count_f1"][i])] for i in range(self.B)]
        pred = []
        for i in range(self.B):
            if self.per_class:
                sem = h["sem_prob"]
                pred.append([(ii, corners8[i, r], sem[i, r, ii] * score[i, r])
                             for ii in range(self.meta["num_class"]) for r in range(count[i])])
            else:
                pred.append([(int(h["cls"][i, r]), corners8[i, r], score[i, r]) for r in range(count[i])])
        return pred, pred_mask


def _views(record, layout):
    out = {}
    for name, dtype, shape, off in layout:
        n = int(np.prod(shape, dtype=np.int64)) * _NUMPY[dtype].itemsize
        out[name] = record[off:off + n].view(dtype).view(shape)
    return out


def _record_for(out, kind, B, K, device, **kw):
    meta = kw.pop("meta")
    if out is None:
        return Detections(kind, B, K, device, meta=meta, **kw), True
    if not isinstance(out, Detections) or not out.matches(kind, B, K, device, **kw):
        raise ValueError(f"ap_helper_pq: `out` is not a {kind} record of this batch's shape, class counts and device")
    out.meta.update(meta)
    return out, False


def detect_predictions(end_points, config_dict, prefix="", out=None):
    """parse_predictions with its results left on the device: -> Detections (kind "boxes").  Same arguments; the inputs under
    `prefix` must be float32 for the call to launch nothing but its own kernels (other dtypes are converted first):
    omnipq_decode_boxes, omnipq_points_in_boxes if remove_empty_box, omnipq_nms3d / _samecls, omnipq_pack_boxes.  No host
    read.  out: a Detections of an earlier call with the same shapes and modes, rewritten in place -- then nothing is
    allocated either (the class mean sizes are uploaded when a record is made, not per call).
    `.to_host()` / `.to_lists()` give parse_predictions' return values."""
    DC = config_dict['dataset_config']
    center = _f32(end_points[f'{prefix}center'], 'center')
    hs = _f32(end_points[f'{prefix}heading_scores'], 'heading_scores')
    hr = _f32(end_points[f'{prefix}heading_residuals'], 'heading_residuals')
    ss = _f32(end_points[f'{prefix}size_scores'], 'size_scores')
    sr = _f32(end_points[f'{prefix}size_residuals'], 'size_residuals')
    sem = _f32(end_points[f'{prefix}sem_cls_scores'], 'sem_cls_scores')
    obj = _f32(end_points[f'{prefix}objectness_scores'], 'objectness_scores')
    B, K = center.shape[:2]
    nh, ns, ncls = hs.shape[-1], ss.shape[-1], sem.shape[-1]
    if max(nh, ns, ncls) > MAX_DECODE_CLASSES or min(nh, ns, ncls) < 1:
        raise ValueError(f"ap_helper_pq: heading bins, size clusters and classes must be in [1, {MAX_DECODE_CLASSES}] "
                         f"(got {nh}, {ns}, {ncls})")
    if K > MAX_PROPOSALS:
        raise ValueError(f"ap_helper_pq: at most {MAX_PROPOSALS} proposals per scene (got {K})")
    if tuple(sr.shape) != (B, K, ns, 3) or tuple(hr.shape) != (B, K, nh) or tuple(obj.shape) != (B, K, 2):
        raise ValueError("ap_helper_pq: heading_residuals (B,K,nh), size_residuals (B,K,ns,3), objectness_scores (B,K,2)")
    means = np.ascontiguousarray(DC.mean_size_arr, dtype=np.float64)
    if means.shape != (ns, 3):
        raise ValueError(f"ap_helper_pq: mean_size_arr must be ({ns}, 3)")
    per_class = bool(config_dict['per_class_proposal'])
    use_3d, cls_nms = bool(config_dict['use_3d_nms']), bool(config_dict['cls_nms'])
    if per_class and int(DC.num_class) > ncls:
        raise ValueError("ap_helper_pq: dataset_config.num_class exceeds the classes of sem_cls_scores")
    det, fresh = _record_for(out, "boxes", B, K, center.device, ncls=ncls, ns=ns, per_class=per_class,
                             meta={"assert_pick": use_3d and not cls_nms, "num_class": int(DC.num_class)})
    f = det.fields
    if fresh:
        f["mean_size"].copy_(torch.from_numpy(means))
    rule = _heading_rule(DC)
    null = ctypes.c_void_p(0)
    _ext._run(_lib.omnipq_decode_boxes, center, B, K, nh, ns, ncls, _ext._ptr(center), _ext._ptr(hs), _ext._ptr(hr),
              _ext._ptr(ss), _ext._ptr(sr), _ext._ptr(sem), _ext._ptr(obj), _ext._ptr(f["mean_size"]),
              1 if rule == "bins" else 0, 0 if use_3d else 1, _ext._ptr(f["heading_cls"]), _ext._ptr(f["size_cls"]),
              _ext._ptr(f["sem_cls"]), _ext._ptr(f["size"]), _ext._ptr(f["heading"]), _ext._ptr(f["obj_prob"]),
              _ext._ptr(f["all_sem_prob"]) if per_class else null, _ext._ptr(f["all_corners8"]), _ext._ptr(f["aabb"]))
    hptr = _ext._ptr(f["heading"]) if rule == "bins" else null           # rule "zero": the axis-aligned path, as above
    vptr = null
    if config_dict['remove_empty_box']:
        pc = _f32(end_points['point_clouds'][:, :, 0:3], 'point_clouds')
        _ext._run(_lib.omnipq_points_in_boxes, pc, B, pc.shape[1], K, _ext._ptr(pc), _ext._ptr(center), _ext._ptr(f["size"]),
                  hptr, 5, _ext._ptr(f["valid"]))
        vptr = _ext._ptr(f["valid"])
    thr, old = float(config_dict['nms_iou']), int(bool(config_dict['use_old_type_nms']))
    if use_3d and cls_nms:
        _ext._run(_lib.omnipq_nms3d_samecls, center, B, K, _ext._ptr(f["aabb"]), _ext._ptr(f["obj_prob"]), vptr,
                  _ext._ptr(f["sem_cls"]), thr, old, _ext._ptr(f["keep"]))
    else:                                            # plain 3D, or bird's-eye view: the decode flattened the extents
        _ext._run(_lib.omnipq_nms3d, center, B, K, _ext._ptr(f["aabb"]), _ext._ptr(f["obj_prob"]), vptr, thr, old,
                  _ext._ptr(f["keep"]))
    _ext._run(_lib.omnipq_pack_boxes, center, B, K, ncls, _ext._ptr(f["keep"]), _ext._ptr(f["obj_prob"]),
              float(config_dict['conf_thresh']), _ext._ptr(f["sem_cls"]), _ext._ptr(f["all_corners8"]),
              _ext._ptr(f["all_sem_prob"]) if per_class else null, _ext._ptr(f["count"]), _ext._ptr(f["index"]),
              _ext._ptr(f["cls"]), _ext._ptr(f["score"]), _ext._ptr(f["corners8"]),
              _ext._ptr(f["sem_prob"]) if per_class else null)
    return det


def detect_quad_predictions(end_points, config_dict, prefix="", out=None):
    """parse_quad_predictions with its results left on the device: -> Detections (kind "quads"), three launches
    (omnipq_parse_quads, omnipq_nms3d, omnipq_pack_quads), no host read, no allocation with `out=`.  The tensor twins
    parse_quad_predictions leaves in end_points are not made."""
    c = _f32(end_points[f'{prefix}quad_center'], "quad_center")
    n = _f32(end_points[f'{prefix}normal_vector'], "normal_vector")
    s = _f32(end_points[f'{prefix}quad_size'], "quad_size")
    sc = _f32(end_points[f'{prefix}quad_scores'], "quad_scores")
    B, K, _ = c.shape
    if n.shape != c.shape or tuple(s.shape) != (B, K, 2) or tuple(sc.shape) != (B, K, 2):
        raise ValueError("ap_helper_pq: quad_center / normal_vector must be (B, K, 3), quad_size and quad_scores (B, K, 2)")
    if K > MAX_PROPOSALS:
        raise ValueError(f"ap_helper_pq: at most {MAX_PROPOSALS} proposals per scene (got {K})")
    det, _ = _record_for(out, "quads", B, K, c.device, meta={"assert_pick": True})
    f = det.fields
    thr = config_dict['nms_iou_quad'] if 'nms_iou_quad' in config_dict else config_dict['nms_iou']
    _ext._run(_lib.omnipq_parse_quads, c, B, K, _ext._ptr(c), _ext._ptr(n), _ext._ptr(s), _ext._ptr(sc), LENGTH,
              _ext._ptr(f["all_corners8"]), _ext._ptr(f["aabb"]), _ext._ptr(f["all_verts4"]), _ext._ptr(f["prob"]))
    _ext._run(_lib.omnipq_nms3d, c, B, K, _ext._ptr(f["aabb"]), _ext._ptr(f["prob"]), ctypes.c_void_p(0), float(thr),
              int(bool(config_dict['use_old_type_nms'])), _ext._ptr(f["keep"]))
    _ext._run(_lib.omnipq_pack_quads, c, B, K, _ext._ptr(f["keep"]), _ext._ptr(f["prob"]), float(config_dict['conf_thresh']),
              QUAD_THRES, _ext._ptr(f["all_corners8"]), _ext._ptr(f["all_verts4"]), _ext._ptr(f["count"]),
              _ext._ptr(f["index"]), _ext._ptr(f["score"]), _ext._ptr(f["corners8"]), _ext._ptr(f["count_f1"]),
              _ext._ptr(f["index_f1"]), _ext._ptr(f["verts4"]))
    return det


# -------------------------------------------------------------------------------------------------- layout F1 on the device
MAX_F1_GT = int(_lib.omnipq_layout_f1_max_gt())                         # g: the library's own limit
MAX_F1_HORIZONTAL = 8                                                   # h (include/omnipq_eval.h)
F1_KEYS = ("tp_wall", "fp", "npos", "tp_horizontal", "scans")


def f1_from_counts(counts, calculated=False):
    """compute_F1's closing expression in Python floats over the integer counts {tp_wall, fp, npos, tp_horizontal}: equal
    counts give bit-equal F1, and npos == 0 raises ZeroDivisionError as the host route does."""
    tp = counts["tp_wall"] + (counts["tp_horizontal"] if calculated else 0)
    fp = counts["fp"]
    p = tp / max((tp + fp), 1e-6)
    r = tp / counts["npos"]
    return 2.0 * p * r / max((p + r), 1e-6)


def _as(t, dtype, shape, keep, name):
    """`t` itself when it already is a contiguous `dtype` tensor of `shape`, otherwise a copy in the staging buffer keep[name]
    (made once per shape): no allocation from the second call on either way"""
    t = t.detach()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"ap_helper_pq: `{name}` must be of shape {tuple(shape)}, not {tuple(t.shape)}")
    if t.dtype == dtype and t.is_contiguous():
        return t
    buf = keep.get(name)
    if buf is None or tuple(buf.shape) != tuple(shape) or buf.device != t.device:
        buf = keep[name] = torch.empty(tuple(shape), device=t.device, dtype=dtype)
    buf.copy_(t)
    return buf


class LayoutF1(object):
    """The layout F1 of an evaluation run, counted on the device (csrc/layout_f1.hip).

        scorer = LayoutF1(device)
        for every batch:   scorer.step(quad_detections, labels)     # two launches, no host read; can be captured
        scorer.f1(), scorer.f1(calculated=True)                     # one copy of five integers each (or read() once)

    acc: int64 (5) device tensor [tp_wall, fp, npos, tp_horizontal, scans], incremented by every step with integer atomics.
    It is a plain tensor: a multi-rank evaluation all-reduces it before reading (the caller's job).  One accumulator serves
    both values of `calculated`."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ap_helper_pq: LayoutF1 counts on the GPU (the HIP path has no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.acc = torch.zeros((5,), device=self.device, dtype=torch.int64)
        self._keep = {}

    def step(self, det, end_points):
        """Adds one batch.  det: the quad Detections of detect_quad_predictions; end_points: the batch's labels ON THE DEVICE,
        as the data loader shapes them -- gt_quad_centers (B, >=g, >=3), gt_normal_vectors (B, >=g, 3), gt_quad_sizes
        (B, >=g, 2), num_total_quads (B, cols) or (B,), horizontal_quads (B, h, 4, 3), g = min(rows, MAX_NUM_QUAD).  The
        ground-truth corners come from omnipq_parse_quads (verts4 alone) into a buffer this object keeps; then one
        omnipq_layout_f1 launch.  float32 / int64 contiguous labels are used where they are, others are first copied into
        buffers kept here; from the second call on nothing is allocated."""
        if not isinstance(det, Detections) or det.kind != "quads":
            raise ValueError("ap_helper_pq: LayoutF1.step takes the quad record of detect_quad_predictions")
        B, K, keep = det.B, det.K, self._keep
        for name in ("gt_quad_centers", "gt_normal_vectors", "gt_quad_sizes", "num_total_quads", "horizontal_quads"):
            t = end_points[name]
            if not torch.is_tensor(t) or t.device != self.device:
                raise RuntimeError(f"ap_helper_pq: `{name}` must be a tensor on {self.device} (LayoutF1 reads nothing from the host)")
        if det.record.device != self.device:
            raise RuntimeError(f"ap_helper_pq: the record is not on {self.device}")
        g = min(int(end_points["gt_quad_centers"].shape[1]), MAX_NUM_QUAD)
        c = _as(end_points["gt_quad_centers"][:, :g, 0:3], _F32, (B, g, 3), keep, "gt_quad_centers")
        n = _as(end_points["gt_normal_vectors"][:, :g], _F32, (B, g, 3), keep, "gt_normal_vectors")
        s = _as(end_points["gt_quad_sizes"][:, :g], _F32, (B, g, 2), keep, "gt_quad_sizes")
        total = end_points["num_total_quads"].reshape(B, -1)
        cols = int(total.shape[1])
        total = _as(total, torch.int64, (B, cols), keep, "num_total_quads")
        hz = end_points["horizontal_quads"]
        h = int(hz.shape[1]) if hz.dim() == 4 else -1
        if h < 0 or h > MAX_F1_HORIZONTAL:
            raise ValueError(f"ap_helper_pq: horizontal_quads must be (B, h, 4, 3) with h <= {MAX_F1_HORIZONTAL}")
        hz = _as(hz, _F32, (B, h, 4, 3), keep, "horizontal_quads")
        gt = keep.get("gt_verts4")
        if gt is None or tuple(gt.shape) != (B, g, 4, 3):
            gt = keep["gt_verts4"] = torch.empty((B, g, 4, 3), device=self.device, dtype=_F32)
        null = ctypes.c_void_p(0)
        _ext._run(_lib.omnipq_parse_quads, c, B, g, _ext._ptr(c), _ext._ptr(n), _ext._ptr(s), null, LENGTH, null, null,
                  _ext._ptr(gt), null)
        _ext._run(_lib.omnipq_layout_f1, c, B, K, _ext._ptr(det.count_f1), _ext._ptr(det.verts4), g, _ext._ptr(gt),
                  _ext._ptr(total), cols, h, _ext._ptr(hz) if h else null, SAME_THRES, null, _ext._ptr(self.acc))
        return self

    def read(self):
        """{tp_wall, fp, npos, tp_horizontal, scans} as Python ints: ONE device-to-host copy (it waits for the steps queued
        before it on the current stream)."""
        return dict(zip(F1_KEYS, (int(v) for v in self.acc.cpu().tolist())))

    def f1(self, calculated=False):
        """QUADAPCalculator.compute_F1(calculated) of the scans added so far"""
        return f1_from_counts(self.read(), calculated)

    def reset(self):
        self.acc.zero_()


def _exact_f32(a, name):
    """a as float32, refused when that would round a corner (the device scores f32 corners; the host route would score the
    wider ones, and the two could then disagree)"""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a
    a32 = a.astype(np.float32)
    if not np.array_equal(a32.astype(np.float64), a.astype(np.float64), equal_nan=True):
        raise ValueError(f"ap_helper_pq: {name} are not exactly representable in float32; f1='device' scores float32 "
                         "corners and does not round -- use f1='host' for these lists")
    return a32


class APCalculator(object):
    ''' Calculating Average Precision '''

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None, iou="host"):
        """
        Args:
            ap_iou_thresh: float between 0 and 1.0
                IoU threshold to judge whether a prediction is positive.
            class2type_map: [optional] dict {class_int:class_name}
            iou: "host" (the reference's route, the default) or "device": the box overlaps of compute_metrics on the
                kernels of csrc/eval_iou.hip (eval_det.eval_det_device)
        """
        self.ap_iou_thresh = ap_iou_thresh
        self.class2type_map = class2type_map
        self.iou = _iou_route(iou)
        self.reset()

    def step(self, batch_pred_map_cls, batch_gt_map_cls):
        """ Accumulate one batch of prediction and groundtruth (the outputs of the two parse functions). """
        bsize = len(batch_pred_map_cls)
        assert (bsize == len(batch_gt_map_cls))
        for i in range(bsize):
            self.gt_map_cls[self.scan_cnt] = batch_gt_map_cls[i]
            self.pred_map_cls[self.scan_cnt] = batch_pred_map_cls[i]
            self.scan_cnt += 1

    def compute_metrics(self):
        """ Use accumulated predictions and groundtruths to compute Average Precision. """
        if self.iou == "device":
            return compute_metrics_at(self, (self.ap_iou_thresh,))[0]
        rec, prec, ap = eval_det.eval_det(self.pred_map_cls, self.gt_map_cls, ovthresh=self.ap_iou_thresh,
                                          get_iou_func=eval_det.get_iou_obb)
        return _metrics_dict(rec, ap, self.class2type_map)

    def reset(self):
        self.gt_map_cls = {}          # {scan_id: [(classname, bbox)]}
        self.pred_map_cls = {}        # {scan_id: [(classname, bbox, score)]}
        self.scan_cnt = 0


def _iou_route(iou):
    if iou not in ("host", "device"):
        raise ValueError(f"ap_helper_pq: iou must be 'host' or 'device', not {iou!r}")
    return iou


def compute_metrics_at(calculator, thresholds):
    """The metric dicts of `calculator.compute_metrics()` at every IoU threshold of `thresholds`, from ONE pass over the box
    overlaps of its accumulated lists (they do not depend on the threshold; the reference keeps one calculator per
    threshold and computes them once each).  The pass runs where the calculator's `iou` says: "device" on the kernels of
    csrc/eval_iou.hip, "host" through eval_det.box3d_iou."""
    thresholds = list(thresholds)
    if calculator.iou == "device":
        triples = eval_det.eval_det_device(calculator.pred_map_cls, calculator.gt_map_cls, ovthresh=thresholds)
    else:
        pack = eval_det.pack_segments(calculator.pred_map_cls, calculator.gt_map_cls)
        ovmax, jmax = eval_det.best_on_host(pack)
        triples = [eval_det.eval_from_best(pack, ovmax, jmax, t) for t in thresholds]
    return [_metrics_dict(rec, ap, calculator.class2type_map) for rec, _, ap in triples]


def _metrics_dict(rec, ap, class2type_map):
    ret_dict = {}
    for key in sorted(ap.keys()):
        clsname = class2type_map[key] if class2type_map else str(key)
        ret_dict['%s Average Precision' % (clsname)] = ap[key]
    ret_dict['mAP'] = np.mean(list(ap.values()))
    rec_list = []
    for key in sorted(ap.keys()):
        clsname = class2type_map[key] if class2type_map else str(key)
        last = rec[key][-1] if np.ndim(rec[key]) and len(rec[key]) else 0
        ret_dict['%s Recall' % (clsname)] = last
        rec_list.append(last)
    ret_dict['AR'] = np.mean(rec_list)
    return ret_dict


class QUADAPCalculator(object):
    ''' Average precision and F1 of the predicted layout quads, accumulated over the scans of an evaluation run '''

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None, logger=None, logger_i=None, iou="host", f1="host"):
        """
        Args:
            ap_iou_thresh: float between 0 and 1.0
                IoU threshold to judge whether a prediction is positive.
            class2type_map: [optional] dict {class_int:class_name}
            iou: "host" (the default) or "device", as for APCalculator
            f1: "host" (the default) or "device": compute_F1 counts the accumulated lists with one launch of
                omnipq_layout_f1 (csrc/layout_f1.hip) instead of walking them in Python
        """
        self.ap_iou_thresh = ap_iou_thresh
        self.class2type_map = class2type_map
        self.iou = _iou_route(iou)
        if f1 not in ("host", "device"):
            raise ValueError(f"ap_helper_pq: f1 must be 'host' or 'device', not {f1!r}")
        self.f1 = f1
        self.logger = logger
        self.I = logger_i
        self.reset()

    def step(self, batch_pred_map_cls, batch_gt_map_cls, batch_pred_corners_list, batch_gt_corners_list,
             batch_gt_horizontal_list):
        """ Accumulate one batch of predictions and ground truths (the outputs of the two parse functions and the batch's
        `horizontal_quads`). """
        bsize = len(batch_pred_map_cls)
        assert (bsize == len(batch_gt_map_cls))
        for i in range(bsize):
            self.gt_map_cls[self.scan_cnt] = batch_gt_map_cls[i]
            self.pred_map_cls[self.scan_cnt] = batch_pred_map_cls[i]
            self.pred_corners[self.scan_cnt] = batch_pred_corners_list[i]
            self.gt_corners[self.scan_cnt] = batch_gt_corners_list[i]
            self.horizontal_corners[self.scan_cnt] = batch_gt_horizontal_list[i]
            self.scan_cnt += 1

    def compute_metrics(self):
        """ Average precision / recall of the accumulated quads as oriented boxes (IoU of get_iou_obb). """
        if self.iou == "device":
            return compute_metrics_at(self, (self.ap_iou_thresh,))[0]
        rec, prec, ap = eval_det.eval_det(self.pred_map_cls, self.gt_map_cls, ovthresh=self.ap_iou_thresh,
                                          get_iou_func=eval_det.get_iou_obb)
        return _metrics_dict(rec, ap, self.class2type_map)

    def reset(self):
        self.gt_map_cls = {}          # {scan_id: [(classname, bbox)]}
        self.pred_map_cls = {}        # {scan_id: [(classname, bbox, score)]}
        self.pred_corners = {}
        self.gt_corners = {}
        self.horizontal_corners = {}
        self.scan_cnt = 0

    def same_point(self, pred, gt):
        return np.linalg.norm(np.asarray(pred) - np.asarray(gt)) <= SAME_THRES

    def compute_correctness(self, pred_corner, all_gt, is_embed=False):
        """A predicted quad is correct when all four corners lie within SAME_THRES of a ground-truth quad's corners, in
        the same order or with the two corners of each edge swapped (the normal's sign is not evaluated)."""
        if len(all_gt) == 0:
            return False
        p = np.asarray([np.asarray(c, dtype=np.float64) for c in pred_corner])              # (4, 3)
        g = np.asarray([np.asarray(c, dtype=np.float64) for c in all_gt])                   # (G, 4, 3)
        same = np.linalg.norm(p[None] - g, axis=-1) <= SAME_THRES
        swapped = np.linalg.norm(p[None] - g[:, [1, 0, 3, 2]], axis=-1) <= SAME_THRES
        return bool((same.all(1) | swapped.all(1)).any())

    def contain_point(self, pointlist, point):
        for p in pointlist:
            if self.same_point(p, point):
                return True, p
        return False, None

    def get_ceiling_and_floor(self, pred_corners):
        """Corner lists of the ceiling (corners 0, 1 of every quad) and the floor (corners 2, 3); a corner that coincides
        with one already listed is appended as the midpoint of the two (the reference appends, it does not merge)."""
        ceilings, floors = [], []
        for quad_corner in pred_corners:
            for i, lst in ((0, ceilings), (1, ceilings), (2, floors), (3, floors)):
                contain, p = self.contain_point(lst, quad_corner[i])
                lst.append(quad_corner[i] if not contain else (p + quad_corner[i]) / 2)
        return ceilings, floors

    def compute_F1(self, calculated=False, is_ema=False):
        """F1 of the accumulated quads; with `calculated` the ceiling and the floor deduced from the predicted walls are
        scored against the scan's horizontal ground-truth quads (true positives only, as in the reference).
        get_ceiling_and_floor appends one entry per visited corner in both of its branches, so the `len(...) == 4` tests
        below hold exactly when the scan has two predicted quads."""
        if self.f1 == "device":
            return f1_from_counts(self.f1_counts_device(), calculated)
        tp = fp = 0
        npos = sum(len(self.gt_corners[i]) for i in range(self.scan_cnt))
        for i in range(self.scan_cnt):
            all_pred_corners = self.pred_corners[i]
            all_gt_corners = self.gt_corners[i]
            horizontal = self.horizontal_corners[i]
            horizontal = horizontal.detach().cpu().numpy() if torch.is_tensor(horizontal) else np.asarray(horizontal)
            for pred_corner in all_pred_corners:
                if self.compute_correctness(pred_corner, all_gt_corners):
                    tp += 1
                else:
                    fp += 1
            if calculated:
                ceilings, floors = self.get_ceiling_and_floor(all_pred_corners)
                if len(ceilings) == 4 and self.compute_correctness(ceilings, horizontal, True):
                    tp += 1
                if len(floors) == 4 and self.compute_correctness(floors, horizontal):
                    tp += 1
        p = tp / max((tp + fp), 1e-6)
        r = tp / npos
        return 2.0 * p * r / max((p + r), 1e-6)

    def f1_counts_device(self, device=None):
        """{tp_wall, fp, npos, tp_horizontal, scans} of the accumulated lists from ONE omnipq_layout_f1 launch: the lists are
        padded into arrays with b = scan_cnt and num_total_cols = 1 (a scan's ground-truth list is already cut, so its count
        is its length), the per-scene rows come back in one copy and are summed here.  Refuses (ValueError) corners that are
        not exactly float32 -- they are not rounded -- lists of more than MAX_PROPOSALS quads, more than MAX_F1_GT
        ground-truth quads and scans whose `horizontal` differ in their row count or exceed MAX_F1_HORIZONTAL rows."""
        b = self.scan_cnt
        counts = dict.fromkeys(F1_KEYS, 0)
        if b == 0:
            return counts
        k = max(max(len(self.pred_corners[i]) for i in range(b)), 1)
        g = max(max(len(self.gt_corners[i]) for i in range(b)), 1)
        if k > MAX_PROPOSALS:
            raise ValueError(f"ap_helper_pq: f1='device' takes at most {MAX_PROPOSALS} predicted quads per scan (got {k})")
        if g > MAX_F1_GT:
            raise ValueError(f"ap_helper_pq: f1='device' takes at most {MAX_F1_GT} ground-truth quads per scan (got {g})")
        hz = []
        for i in range(b):
            one = self.horizontal_corners[i]
            one = one.detach().cpu().numpy() if torch.is_tensor(one) else np.asarray(one)
            hz.append(_exact_f32(one, "horizontal quads").reshape(-1, 4, 3))
        h = hz[0].shape[0]
        if any(x.shape[0] != h for x in hz) or h > MAX_F1_HORIZONTAL:
            raise ValueError(f"ap_helper_pq: f1='device' needs the same number (<= {MAX_F1_HORIZONTAL}) of horizontal quads "
                             "for every scan: padding rows are scored like any other row")
        verts = np.zeros((b, k, 4, 3), np.float32)
        gt = np.zeros((b, g, 4, 3), np.float32)
        count = np.zeros((b,), np.int32)
        total = np.zeros((b, 1), np.int64)
        for i in range(b):
            for arr, lst, n, name in ((verts, self.pred_corners[i], count, "predicted corners"),
                                      (gt, self.gt_corners[i], total, "ground-truth corners")):
                n[i] = len(lst)
                if len(lst):
                    arr[i, :len(lst)] = _exact_f32(np.stack([np.asarray(q) for q in lst]), name).reshape(-1, 4, 3)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        d = [torch.from_numpy(a).to(dev) for a in (count, verts, gt, total)]
        dh = torch.from_numpy(np.ascontiguousarray(np.stack(hz))).to(dev) if h else None
        rows = torch.empty((b, 4), device=dev, dtype=_I32)
        null = ctypes.c_void_p(0)
        _ext._run(_lib.omnipq_layout_f1, rows, b, k, _ext._ptr(d[0]), _ext._ptr(d[1]), g, _ext._ptr(d[2]), _ext._ptr(d[3]), 1,
                  h, null if dh is None else _ext._ptr(dh), SAME_THRES, _ext._ptr(rows), null)
        sums = rows.cpu().numpy().astype(np.int64).sum(0)
        counts.update(zip(F1_KEYS, (int(v) for v in sums)), scans=b)
        return counts
