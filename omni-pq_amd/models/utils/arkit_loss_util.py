"""ARKit physical-constraint loss of Omni-PQ -- the reference's `models/utils/arkit_loss_util.py` on the kernels of
csrc/arkit_pc.hip (include/omnipq_semi.h, which states the mathematics).  Same name, argument order and return pair:

    get_arkit_pc_loss(end_points, batch_data_unlabeled, config)            arkit_loss_util.py:5-52, train.py:537
        -> (pc_loss, collisions)

The ground-truth boxes of the UNLABELLED scenes must not poke through the quads predicted for them: every footprint corner of
every box against every `last_` quad of the scene whose score passes 0.1.  The reference loops over B x 256 quads in Python,
with a host read (`if quad_scores[b, k] > 0.1`) and about twenty small ops per quad.  Here it is

    omnipq_arkit_pc         2 launches  (one workgroup per scene, one thread per quad; the sum over the scenes, in scene order)
    omnipq_arkit_pc_grad    1 launch    (gradients to last_quad_center[..., :2] and last_normal_vector[..., :2])

with no host read anywhere: it can be part of the criterion of `train_step.CapturedStep`.  The same inputs give the same
bits (f64 sums in a fixed order, no float atomics).  There is no CPU path.

Differences from the reference, on purpose:
  * a scene without boxes (`num_gt_boxes[s, 0] <= 0`) contributes 0 to both values; the reference divides 0 by 0 and the total
    is NaN as soon as one quad of that scene passes the gate.
  * label rows at and beyond the scene's count are never read (they may hold anything, NaN included).
  * both return values are always 0-dim float32 device tensors; the reference returns Python `0.0` / `0` when no quad passes.
  * per pair everything is computed in float64 from the float32 inputs; the reference computes in float32.
  * the full batch must hold exactly twice the unlabelled batch (`[batch_size:]` is then the unlabelled half); the reference
    mis-indexes silently otherwise.  At most MAX_BOXES label rows per scene.
  * every input is left untouched.
"""
import torch

from pointnet2 import _ext

_lib = _ext._lib

GATE = 0.1                             # :45; csrc/arkit_pc.hip: kArkGate
COLLISION = 1e-4                       # loss_helper_pq.py:349; kArkHit
MAX_BOXES = _ext.const("OMNIPQ_ARKIT_MAX_BOXES")
RECORD_INTS = _ext.const("OMNIPQ_ARKIT_RECORD_INTS")
RECORD_KEYS = ("gate", "rev", "inside", "live", "collisions")
PREFIX = "last_"                       # :8
PREDICTION_KEYS = ("quad_center", "normal_vector", "quad_size", "quad_scores")      # in the order of the C ABI


def _f32_all(tensors):
    """Contiguous float32 versions of CUDA tensors; the 16-bit ones are converted by ONE multi-tensor copy."""
    out = [t.detach() for t in tensors]
    narrow = [i for i, t in enumerate(out) if t.dtype != torch.float32]
    if narrow:
        wide = [torch.empty(out[i].shape, device=out[i].device, dtype=torch.float32) for i in narrow]
        torch._foreach_copy_(wide, [out[i] for i in narrow])
        for i, t in zip(narrow, wide):
            out[i] = t
    return [t.contiguous() for t in out]


class _ArkitPc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quad_center, normal_vector, quad_size, quad_scores, center_label, size_label, counts, stride):
        qc, nv, qs, sc, cl, sl = _f32_all((quad_center, normal_vector, quad_size, quad_scores, center_label, size_label))
        Bu, K2 = cl.shape[0], cl.shape[1]
        Q = qc.shape[1]
        dev = qc.device
        record = torch.empty((Bu, Q, RECORD_INTS), device=dev, dtype=torch.int32)
        scene_sums = torch.empty((Bu, 2), device=dev, dtype=torch.float64)
        out = torch.empty(2, device=dev, dtype=torch.float32)
        shape = (qc.shape[0] - Bu, Bu, Q, K2)
        ptrs = tuple(_ext._ptr(t) for t in (qc, nv, qs, sc, cl, sl, counts))
        _ext._run(_lib.omnipq_arkit_pc, qc, *shape, *ptrs, stride, _ext._ptr(record), _ext._ptr(scene_sums), _ext._ptr(out))
        ctx.keep = (qc, nv, qs, sc, cl, sl, counts, record)
        ctx.cfg = (shape, stride, quad_center.dtype, normal_vector.dtype)
        ctx.mark_non_differentiable(record)
        return out, record

    @staticmethod
    def backward(ctx, g_out, _g_record):
        qc, nv, qs, sc, cl, sl, counts, record = ctx.keep
        shape, stride, dt_qc, dt_nv = ctx.cfg
        g = g_out.float().contiguous()                          # [0]: dLoss/dloss; the collision count takes no gradient
        g_qc, g_nv = torch.empty_like(qc), torch.empty_like(nv)
        ptrs = tuple(_ext._ptr(t) for t in (qc, nv, qs, sc, cl, sl, counts))
        _ext._run(_lib.omnipq_arkit_pc_grad, qc, *shape, *ptrs, stride, _ext._ptr(record), _ext._ptr(g), _ext._ptr(g_qc),
                  _ext._ptr(g_nv))
        grads = [g_qc, g_nv]
        narrow = [i for i, dt in enumerate((dt_qc, dt_nv)) if dt != torch.float32]
        if narrow:                                              # gradients in the inputs' dtype: one multi-tensor copy
            cast = [torch.empty(grads[i].shape, device=g_qc.device, dtype=(dt_qc, dt_nv)[i]) for i in narrow]
            torch._foreach_copy_(cast, [grads[i] for i in narrow])
            for i, t in zip(narrow, cast):
                grads[i] = t
        return grads[0], grads[1], None, None, None, None, None, None


def _prepare(end_points, batch_data_unlabeled):
    """-> the arguments of _ArkitPc.apply, validated"""
    gt_centers, gt_sizes = batch_data_unlabeled["center_label"], batch_data_unlabeled["size_label"]
    box_nums = batch_data_unlabeled["num_gt_boxes"]
    preds = [end_points[PREFIX + k] for k in PREDICTION_KEYS]
    for name, t in zip(PREDICTION_KEYS + ("center_label", "size_label", "num_gt_boxes"), preds + [gt_centers, gt_sizes, box_nums]):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"arkit_loss_util: {name} must be a CUDA tensor (there is no CPU path)")
    if gt_centers.dim() != 3 or gt_centers.shape[2] != 3 or tuple(gt_sizes.shape) != tuple(gt_centers.shape):
        raise ValueError(f"arkit_loss_util: center_label and size_label must have one shape (Bu, K2, 3), not "
                         f"{tuple(gt_centers.shape)} and {tuple(gt_sizes.shape)}")
    Bu, K2 = gt_centers.shape[0], gt_centers.shape[1]
    if K2 < 1 or K2 > MAX_BOXES:
        raise ValueError(f"arkit_loss_util: K2 = {K2} label rows per scene outside [1, {MAX_BOXES}] (a scene's boxes live in LDS)")
    if box_nums.dim() != 2 or box_nums.shape[0] != Bu or box_nums.shape[1] < 1 or box_nums.is_floating_point():
        raise ValueError(f"arkit_loss_util: num_gt_boxes must be an integer tensor of shape ({Bu}, >= 1), not "
                         f"{tuple(box_nums.shape)} {box_nums.dtype}")
    qc = preds[0]
    if qc.dim() != 3 or qc.shape[1] < 1:
        raise ValueError(f"arkit_loss_util: {PREFIX}quad_center must have shape (Bt, Q, 3), not {tuple(qc.shape)}")
    Bt, Q = qc.shape[0], qc.shape[1]
    if Bt != 2 * Bu:
        raise ValueError(f"arkit_loss_util: the predictions hold {Bt} scenes, the unlabelled batch {Bu}: the loss reads the scenes "
                         f"[{Bu}:] and needs exactly twice the unlabelled batch")
    for name, t, last in zip(PREDICTION_KEYS, preds, (3, 3, 2, 2)):
        if tuple(t.shape) != (Bt, Q, last):
            raise ValueError(f"arkit_loss_util: {PREFIX + name} must have shape {(Bt, Q, last)}, not {tuple(t.shape)}")
    counts = box_nums.detach()
    if counts.dtype != torch.int64:
        counts = counts.long()
    counts = counts[..., 0]                                     # a strided view: the kernel reads it with its stride
    stride = int(counts.stride(0)) if Bu > 1 else 1
    if stride < 1:
        counts, stride = counts.contiguous(), 1
    return (*preds, gt_centers, gt_sizes, counts, stride)


def _zeros(end_points):
    zero = torch.zeros((), device=end_points[PREFIX + "quad_center"].device, dtype=torch.float32)
    return zero, zero.clone()


def get_arkit_pc_loss(end_points, batch_data_unlabeled, config=None):
    """-> (pc_loss, collisions): 0-dim float32 device tensors.  Reads `last_quad_center`, `last_normal_vector` (Bt, Q, 3),
    `last_quad_size`, `last_quad_scores` (Bt, Q, 2) of the scenes [Bu:] from `end_points` and `center_label`, `size_label`
    (Bu, K2, 3), `num_gt_boxes` (Bu, >= 1) integer, column 0 = the scene's number of boxes) from `batch_data_unlabeled`; Bt must
    be 2 Bu.  pc_loss is differentiable with respect to `last_quad_center[..., :2]` and `last_normal_vector[..., :2]` of the
    scenes [Bu:] (the gradient tensors are zero elsewhere); nothing flows to the scores, the sizes or the labels.  16-bit
    inputs are computed in float32 and receive gradients in their own dtype.  Writes nothing.  `config` is accepted and
    unused, as in the reference."""
    args = _prepare(end_points, batch_data_unlabeled)
    if args[4].shape[0] == 0:
        return _zeros(end_points)
    out, _ = _ArkitPc.apply(*args)
    loss, collisions = out.unbind(0)
    return loss, collisions.detach()


def decisions(end_points, batch_data_unlabeled, config=None):
    """What the forward decided, for tests and diagnostics: a dict of (Bu, Q) int32 device tensors -- `gate` (the quad's score
    passes), `rev` (its normal was turned inwards), `inside` (corners whose projection lies on the quad), `live` (those of them
    behind it: delta < 0), `collisions` (those deeper than 1e-4).  A quad that does not pass the gate has zeros throughout."""
    args = _prepare(end_points, batch_data_unlabeled)
    with torch.no_grad():
        record = _ArkitPc.apply(*args)[1]
    return {k: record[..., i] for i, k in enumerate(RECORD_KEYS)}
