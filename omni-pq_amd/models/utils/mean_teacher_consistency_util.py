"""Mean-teacher consistency loss of Omni-PQ -- the reference's `models/utils/mean_teacher_consistency_util.py` on the
kernels of csrc/consistency.hip (include/omnipq_semi.h, which states the mathematics).  Same name, arguments, `end_points`
keys and return values:

    get_consistency_loss(end_points, ema_end_points, config)            mean_teacher_consistency_util.py:201-270
        -> (consistency_loss + quad_consistency_loss_sum, end_points)

The reference runs about sixty small PyTorch ops per prediction head and kind, fourteen times per step, with `nonzero` and
per-scene Python list comprehensions.  Here all seven heads and both kinds are

    omnipq_mt_consistency         3 launches  (rows: one workgroup per scene, head and kind; clip: the 0.85 quantiles, masks
                                               and masked sums; a one-wave fold into the ten terms)
    omnipq_mt_consistency_grad    1 launch    (every gradient row written once, gathered over the stored assignments and masks)

with no host read anywhere: it can be part of the criterion of `train_step.CapturedStep(teacher=...,
teacher_to_criterion=True)`.  The same inputs give the same bits (f64 sums in a fixed order, integer radix selection for the
quantiles, no float atomics).  There is no CPU path.

Differences from the reference, on purpose:
  * the reference flips the TEACHER's `*center` / `*quad_center` tensors in place (:32-35, :70-73) -- a second call on the same
    `ema_end_points` would flip them back.  This implementation leaves every input untouched; the aligned centres are in
    `end_points['*ema_center']` / `['*ema_center_quad']` as in the reference.
  * `*ema_assignment_confidence` / `*ema_assignment_quad_confidence` are stored detached (the reference stores the live
    softmax output); the gradient through the confidences reaches the scores all the same, inside the one autograd node.
  * per row everything is computed in float64 from the float32 inputs; the reference computes in float32.
  * the number of object and quad proposals must be equal (one `k` in the C ABI), at most MAX_K, and B * K at most MAX_ROWS.
The teacher's normals are NOT aligned with the student's frame -- the reference does not align them either.
The mean-teacher ramp-up weight (train.py:530-532) is a host scalar the caller multiplies the result with.
"""
import ctypes

import numpy as np
import torch

from pointnet2 import _ext

_lib = _ext._lib

EMA_CLIP = 0.85                        # :17; csrc/consistency.hip: kMtClip
PREFIXES = ("last_", "proposal_") + tuple(f"{i}head_" for i in range(5))      # :228
MAX_PREFIXES = _ext.const("OMNIPQ_MT_MAX_PREFIXES")
MAX_CLASSES = _ext.const("OMNIPQ_MT_MAX_CLASSES")
MAX_K = _ext.const("OMNIPQ_MT_MAX_K")
MAX_ROWS = _ext.const("OMNIPQ_MT_MAX_ROWS")
TERMS = _ext.const("OMNIPQ_MT_TERMS")
# the nine end_points keys of :258-267, in the order of the kernel's terms; terms[9] is the returned total
TERM_KEYS = ("center_consistency_loss", "class_consistency_loss", "size_consistency_loss", "consistency_loss",
             "quad_center_consistency_loss_sum", "quad_class_consistency_loss_sum", "quad_normal_consistency_loss_sum",
             "quad_size_consistency_loss_sum", "quad_consistency_loss_sum")
# per prefix, the fields of omnipq_mt_desc (the teacher's with a `t_` in front) in the order the tensors are handed to
# _Consistency; the student's size_scores take no gradient (arg-max)
STUDENT_KEYS = ("center", "objectness_scores", "sem_cls_scores", "size_scores", "size_residuals", "quad_center", "quad_scores",
                "normal_vector", "quad_size")
TEACHER_KEYS = ("center", "sem_cls_scores", "size_scores", "size_residuals", "quad_center", "quad_scores", "normal_vector",
                "quad_size")
GRAD_KEYS = tuple(k for k in STUDENT_KEYS if k != "size_scores")

_Desc = _ext.struct("omnipq_mt_desc")
_Grads = _ext.struct("omnipq_mt_grads")


def _f32(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mean_teacher_consistency_util: {name} must be a CUDA tensor (there is no CPU path)")
    return t.detach().float().contiguous()


def _f32_all(tensors, name):
    """Contiguous float32 versions of CUDA tensors.  The 16-bit ones are converted by ONE multi-tensor copy: a `.float()` each
    is a launch each, about 120 of them per call under autocast."""
    out = []
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"mean_teacher_consistency_util: {name} must be a CUDA tensor (there is no CPU path)")
        out.append(t.detach())
    narrow = [i for i, t in enumerate(out) if t.dtype != torch.float32]
    if narrow:
        wide = [torch.empty(out[i].shape, device=out[i].device, dtype=torch.float32) for i in narrow]
        torch._foreach_copy_(wide, [out[i] for i in narrow])
        for i, t in zip(narrow, wide):
            out[i] = t
    return [t.contiguous() for t in out]


_mean_size_cache = {}


def _mean_size(config, device):
    """config.mean_size_arr (ns, 3) as a float32 device tensor (:131-132), uploaded once per array and device: an upload
    inside a graph capture would be a host read of its own"""
    arr = np.ascontiguousarray(np.asarray(config.mean_size_arr, dtype=np.float32))
    key = (str(device), arr.shape, arr.tobytes())
    if key not in _mean_size_cache:
        _mean_size_cache[key] = torch.from_numpy(arr.copy()).to(device)
    return _mean_size_cache[key]


class _Consistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, shape, aug, teacher, *student):
        P, B, K, nc, ns = shape
        dev = student[0].device
        tensors = _f32_all(student, "a student tensor")
        desc = _Desc(P, B, K, nc, ns)
        for i, t in enumerate(tensors):
            getattr(desc, STUDENT_KEYS[i % len(STUDENT_KEYS)])[i // len(STUDENT_KEYS)] = t.data_ptr()
        for i, t in enumerate(teacher):
            getattr(desc, "t_" + TEACHER_KEYS[i % len(TEACHER_KEYS)])[i // len(TEACHER_KEYS)] = t.data_ptr()
        desc.flip_x, desc.flip_y, desc.rot_mat, desc.scale, desc.mean_size = (t.data_ptr() for t in aug)
        ema_center = torch.empty((P, 2, B, K, 3), device=dev, dtype=torch.float32)
        assignment = torch.empty((P, 2, B, K), device=dev, dtype=torch.int64)
        confidence = torch.empty((P, 2, B, K), device=dev, dtype=torch.float32)
        terms = torch.empty(TERMS, device=dev, dtype=torch.float32)
        nbytes = int(_lib.omnipq_mt_consistency_workspace_bytes(P, B, K))
        workspace = torch.empty(max(nbytes, 256), device=dev, dtype=torch.uint8)
        _ext._run(_lib.omnipq_mt_consistency, tensors[0], ctypes.byref(desc), _ext._ptr(ema_center), _ext._ptr(assignment),
                  _ext._ptr(confidence), _ext._ptr(workspace), _ext._ptr(terms))
        ctx.keep = (desc, tensors, teacher, aug, workspace)
        ctx.dtypes = [t.dtype for t in student]
        ctx.mark_non_differentiable(ema_center, assignment, confidence, workspace)
        return terms, ema_center, assignment, confidence, workspace

    @staticmethod
    def backward(ctx, g_terms, *_unused):
        desc, tensors, _teacher, _aug, workspace = ctx.keep
        g = g_terms.float().contiguous()
        grads, out = _Grads(), []
        for i, t in enumerate(tensors):
            key = STUDENT_KEYS[i % len(STUDENT_KEYS)]
            if key == "size_scores":
                out.append(None)
                continue
            buf = torch.empty_like(t)
            getattr(grads, key)[i // len(STUDENT_KEYS)] = buf.data_ptr()
            out.append(buf)
        _ext._run(_lib.omnipq_mt_consistency_grad, tensors[0], ctypes.byref(desc), _ext._ptr(workspace), _ext._ptr(g),
                  ctypes.byref(grads))
        narrow = [i for i, (b, dt) in enumerate(zip(out, ctx.dtypes)) if b is not None and dt != torch.float32]
        if narrow:                                   # gradients in the inputs' dtype: one multi-tensor copy, as on the way in
            cast = [torch.empty(out[i].shape, device=out[i].device, dtype=ctx.dtypes[i]) for i in narrow]
            torch._foreach_copy_(cast, [out[i] for i in narrow])
            for i, t in zip(narrow, cast):
                out[i] = t
        return (None, None, None) + tuple(out)


def _prepare(end_points, ema_end_points, config, prefixes):
    """-> the arguments of _Consistency.apply, validated"""
    prefixes = tuple(prefixes)
    P = len(prefixes)
    if P < 1 or P > MAX_PREFIXES:
        raise ValueError(f"mean_teacher_consistency_util: {P} prefixes outside [1, {MAX_PREFIXES}]")
    first = end_points[prefixes[0] + "center"]
    if not first.is_cuda:
        raise RuntimeError("mean_teacher_consistency_util: end_points must hold CUDA tensors (there is no CPU path)")
    B, K = first.shape[0], first.shape[1]
    nc = end_points[prefixes[0] + "sem_cls_scores"].shape[2]
    ns = end_points[prefixes[0] + "size_scores"].shape[2]
    if K < 1 or K > MAX_K or B * K > MAX_ROWS:
        raise ValueError(f"mean_teacher_consistency_util: K = {K} outside [1, {MAX_K}] or B * K = {B * K} above {MAX_ROWS} "
                         "(a scene's proposals and a call's clipped values live in LDS)")
    if not (1 <= nc <= MAX_CLASSES and 1 <= ns <= MAX_CLASSES):
        raise ValueError(f"mean_teacher_consistency_util: {nc} classes / {ns} size clusters outside [1, {MAX_CLASSES}]")
    shapes = {"center": (B, K, 3), "objectness_scores": (B, K, 2), "sem_cls_scores": (B, K, nc), "size_scores": (B, K, ns),
              "size_residuals": (B, K, ns, 3), "quad_center": (B, K, 3), "quad_scores": (B, K, 2), "normal_vector": (B, K, 3),
              "quad_size": (B, K, 2)}
    student, teacher = [], []
    for p in prefixes:
        for k in STUDENT_KEYS:
            t = end_points[p + k]
            if tuple(t.shape) != shapes[k]:
                raise ValueError(f"mean_teacher_consistency_util: {p + k} must have shape {shapes[k]}, not {tuple(t.shape)}")
            student.append(t)
        for k in TEACHER_KEYS:
            t = ema_end_points[p + k]
            if tuple(t.shape) != shapes[k]:
                raise ValueError(f"mean_teacher_consistency_util: the teacher's {p + k} must have shape {shapes[k]}, "
                                 f"not {tuple(t.shape)}")
            teacher.append(t)
    flips = []
    for key in ("flip_x_axis", "flip_y_axis"):
        t = end_points[key]
        if not t.is_cuda or t.numel() != B:
            raise ValueError(f"mean_teacher_consistency_util: {key} must be a CUDA tensor of {B} elements")
        flips.append((t.detach().reshape(B) != 0).to(torch.int32).contiguous())
    rot, scale = _f32(end_points["rot_mat"], "rot_mat"), _f32(end_points["scale"], "scale")
    if tuple(rot.shape) != (B, 3, 3) or scale.numel() != B:
        raise ValueError("mean_teacher_consistency_util: rot_mat must be (B, 3, 3) and scale must have B elements")
    mean_size = _mean_size(config, first.device)
    if tuple(mean_size.shape) != (ns, 3):
        raise ValueError(f"mean_teacher_consistency_util: config.mean_size_arr must be ({ns}, 3)")
    aug = (flips[0], flips[1], rot, scale.reshape(B), mean_size)
    return (P, B, K, nc, ns), aug, tuple(_f32_all(teacher, "a teacher tensor")), student


def get_consistency_loss(end_points, ema_end_points, config, prefixes=PREFIXES):
    """-> (consistency_loss + quad_consistency_loss_sum: a 0-dim float32 device tensor, end_points).

    Reads, for every prefix, the student's `center`, `objectness_scores`, `sem_cls_scores`, `size_scores`, `size_residuals`,
    `quad_center`, `quad_scores`, `normal_vector`, `quad_size` from `end_points` and the teacher's (without
    `objectness_scores`) from `ema_end_points`; `flip_x_axis` (B,), `flip_y_axis` (B,), `rot_mat` (B, 3, 3) and `scale` (B
    elements in any shape) from `end_points`, where train.py:526-529 puts them; `config.mean_size_arr` (ns, 3).  Differentiable
    with respect to the student's tensors except `size_scores`; nothing flows to the teacher.  16-bit inputs are computed in
    float32 and receive gradients in their own dtype.

    Writes to `end_points` what the reference writes: per prefix `ema_center`, `ema_assignment` (int64),
    `ema_assignment_confidence` and their `_quad` twins (`ema_center_quad`, `ema_assignment_quad`,
    `ema_assignment_quad_confidence`), and the nine keys of TERM_KEYS.  No input is modified (see the module docstring).
    prefixes (extension): the prediction heads to run over, at most MAX_PREFIXES."""
    prefixes = tuple(prefixes)
    if end_points[prefixes[0] + "center"].shape[0] == 0:
        zero = torch.zeros((), device=end_points[prefixes[0] + "center"].device, dtype=torch.float32)
        for key in TERM_KEYS:
            end_points[key] = zero.clone()
        return zero, end_points
    shape, aug, teacher, student = _prepare(end_points, ema_end_points, config, prefixes)
    terms, ema_center, assignment, confidence, _ = _Consistency.apply(shape, aug, teacher, *student)
    for i, p in enumerate(prefixes):
        end_points[p + "ema_center"], end_points[p + "ema_center_quad"] = ema_center[i, 0], ema_center[i, 1]
        end_points[p + "ema_assignment"], end_points[p + "ema_assignment_quad"] = assignment[i, 0], assignment[i, 1]
        end_points[p + "ema_assignment_confidence"] = confidence[i, 0]
        end_points[p + "ema_assignment_quad_confidence"] = confidence[i, 1]
    parts = terms.unbind(0)
    for key, value in zip(TERM_KEYS, parts):
        end_points[key] = value
    return parts[9], end_points


def decisions(end_points, ema_end_points, config, prefixes=PREFIXES):
    """What the forward decided, for tests and diagnostics: a dict of device tensors indexed [prefix, kind (0 objects,
    1 quads)] -- ind1, ind2 (P, 2, B, K) int32; masks (P, 2, 3, B, K) uint8 (kind 0: centre, size, unused; kind 1: centre,
    normal, quad size); cls (P, 2, B, K) int32, the arg-max size classes (index 1: 0 the student's, 1 the teacher's);
    eps (P, 2, 4) float32.  The layout is csrc/consistency.hip: mt_layout."""
    shape, aug, teacher, student = _prepare(end_points, ema_end_points, config, tuple(prefixes))
    with torch.no_grad():
        workspace = _Consistency.apply(shape, aug, teacher, *student)[4]
    P, B, K = shape[:3]
    n, pk = B * K, 2 * P
    off = 0

    def region(count, dtype, view):
        nonlocal off
        size = count * torch.empty((), dtype=dtype).element_size()
        out = workspace[off:off + size].view(dtype).reshape(view)
        off += size
        return out

    region(pk * B, torch.float64, (P, 2, B))
    region(pk * 4, torch.float64, (P, 2, 4))
    region(pk * 3 * n, torch.float32, (P, 2, 3, B, K))
    ind1 = region(pk * n, torch.int32, (P, 2, B, K))
    ind2 = region(pk * n, torch.int32, (P, 2, B, K))
    cls = region(pk * n, torch.int32, (P, 2, B, K))
    eps = region(pk * 4, torch.float32, (P, 2, 4))
    masks = region(pk * 3 * n, torch.uint8, (P, 2, 3, B, K))
    return {"ind1": ind1, "ind2": ind2, "cls": cls, "eps": eps, "masks": masks}
