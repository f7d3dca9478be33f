"""Gamma-mixture guide criterion of Omni-PQ -- the reference's `models/utils/gamma_mixture_loss_util.py` on the kernels of
csrc/gamma_guide.hip (include/omnipq_semi.h).  Same name, arguments, `end_points` keys and four return values:

    gamma_mixture_guide_criterion(end_points, DATASET_CONFIG, config, **kwargs)        gamma_mixture_loss_util.py:130-192
        -> (metric_normal, metric_vertical, metric_size, metric_score), each summed over the scenes and divided by B

The reference picks one quad per scene with `random.choice`, samples 10 000 points with `torch.randint`, runs about sixty
small PyTorch ops and several `.item()` reads per scene and sends the distances through numpy into fit.py's `fit_gamma`
(25 EM steps with scipy.optimize.root).  `fit_gamma` labels the samples with the two gamma densities it builds from its
ARGUMENTS (fit.py:160, :168-173), which the fit never updates: with the call site's arguments (:65) a sample is kept iff its
distance is at most `T_STAR`.  So the criterion is a fixed function of its inputs and of the two draws, and here it is

    omnipq_gm_draw          1 launch    (pick a candidate quad per scene, K sample indices per scene; counter-based hash)
    omnipq_gm_guide         2 launches  (one workgroup per scene; the sum over the scenes, in scene order)
    omnipq_gm_guide_grad    1 launch    (gradients to quad_scores, quad_center, quad_size)

with no host read anywhere: it can be part of the criterion of `train_step.CapturedStep`.  The same inputs and draws give
the same bits (f64 sums in a fixed order, integer radix selection for the quantiles).  There is no CPU path.

Differences from the reference, on purpose:
  * the reference executes `quad_size[0] /= 1.5` IN PLACE on a view of the caller's tensor (:29): after its call,
    `end_points['last_quad_size'][b, pick, 0]` is divided by 1.5 and the consistency loss that runs next sees that.  This
    implementation leaves every input untouched.
  * the `random` / `torch.randint` streams are not reproduced (they cannot be), the distributions are: uniform over the
    candidate quads, uniform with replacement over the points.  The seed is a device counter of its own
    (pointnet2/dropout_state.py, slot "gamma_mixture"), first drawn from torch's generator and advanced once per call.
    The counter is created by the first call on a device: make that call outside a graph capture (the warm-up steps of
    `train_step.CapturedStep` do).
  * the z size candidate (:110, :115) carries the weight `0.` in the reference and is not computed.
"""
import torch

import dropout_state
from pointnet2 import _ext

_lib = _ext._lib

GM_CLIP = 0.85                         # quantile below which a kept point's vertical distance counts (:12, :93)
T_STAR = 0.29961316955346434           # root of 40 e^(-19 t) = 0.45 t: what fit_gamma(a1=2, b1=20, a2=3, b2=1, weight=0.1) keeps
MIN_KEPT = 300                         # fewer kept points: the scene contributes nothing (:78)
DEFAULT_K = 10000                      # :176
MAX_K = _ext.const("OMNIPQ_GM_MAX_K")
RECORD_FLOATS = _ext.const("OMNIPQ_GM_RECORD_FLOATS")
SEED_SLOT = "gamma_mixture"


def _f32(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"gamma_mixture_loss_util: {name} must be a CUDA tensor (there is no CPU path)")
    return t.detach().float().contiguous()


def _i32(t, name, shape, like):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if tuple(t.shape) != shape:
        raise ValueError(f"gamma_mixture_loss_util: {name} must have shape {shape}, not {tuple(t.shape)}")
    return t.detach().to(device=like.device, dtype=torch.int32).contiguous()


def draw(quad_scores, num_points, K=DEFAULT_K):
    """-> (pick (B,) int32, skip (B,) int32, sample_inds (B, K) int32), see omnipq_gm_draw.  Advances the counter."""
    sc = _f32(quad_scores, "quad_scores")
    B, Q, _ = sc.shape
    pick = torch.empty(B, device=sc.device, dtype=torch.int32)
    skip = torch.empty(B, device=sc.device, dtype=torch.int32)
    inds = torch.empty((B, K), device=sc.device, dtype=torch.int32)
    with dropout_state.STATE.use(SEED_SLOT):
        seed = dropout_state.STATE.bump(sc.device)
    _ext._run(_lib.omnipq_gm_draw, sc, B, int(num_points), Q, int(K), _ext._ptr(sc), _ext._ptr(seed), 0, _ext._ptr(pick),
              _ext._ptr(skip), _ext._ptr(inds))
    return pick, skip, inds


class _Guide(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quad_scores, quad_center, quad_size, normal_vector, xyz, normals, pick, skip, sample_inds):
        sc, qc, qs = _f32(quad_scores, "quad_scores"), _f32(quad_center, "quad_center"), _f32(quad_size, "quad_size")
        nv, px, pm = _f32(normal_vector, "normal_vector"), _f32(xyz, "point_clouds"), _f32(normals, "vertex_normals")
        B, N, pitch = px.shape
        Q, K = sc.shape[1], sample_inds.shape[1]
        if tuple(pm.shape) != (B, N, 3) or tuple(sc.shape) != (B, Q, 2) or tuple(qc.shape) != (B, Q, 3) or \
                tuple(nv.shape) != (B, Q, 3) or tuple(qs.shape) != (B, Q, 2):
            raise ValueError("gamma_mixture_loss_util: point_clouds (B, N, >=3), vertex_normals (B, N, 3), quad_scores (B, Q, 2), "
                             "quad_center (B, Q, 3), normal_vector (B, Q, 3), quad_size (B, Q, 2)")
        record = torch.empty((B, RECORD_FLOATS), device=px.device, dtype=torch.float32)
        terms = torch.zeros(4, device=px.device, dtype=torch.float32)
        shape = (B, N, Q, K, pitch)
        ptrs = tuple(_ext._ptr(t) for t in (px, pm, sc, qc, nv, qs))
        _ext._run(_lib.omnipq_gm_guide, px, *shape, *ptrs, _ext._ptr(pick), _ext._ptr(skip) if skip is not None else None,
                  _ext._ptr(sample_inds), _ext._ptr(record), _ext._ptr(terms))
        ctx.keep = (px, pm, sc, qc, nv, qs, pick, sample_inds, record)
        ctx.cfg = (shape, quad_scores.dtype, quad_center.dtype, quad_size.dtype)
        ctx.mark_non_differentiable(record)
        return terms, record

    @staticmethod
    def backward(ctx, g_terms, _g_record):
        px, pm, sc, qc, nv, qs, pick, sample_inds, record = ctx.keep
        shape, dt_sc, dt_qc, dt_qs = ctx.cfg
        g = g_terms.float().contiguous()
        g_sc, g_qc, g_qs = torch.empty_like(sc), torch.empty_like(qc), torch.empty_like(qs)
        if shape[0]:
            ptrs = tuple(_ext._ptr(t) for t in (px, pm, sc, qc, nv, qs, pick, sample_inds, record, g, g_sc, g_qc, g_qs))
            _ext._run(_lib.omnipq_gm_guide_grad, px, *shape, *ptrs)
        return g_sc.to(dt_sc), g_qc.to(dt_qc), g_qs.to(dt_qs), None, None, None, None, None, None


def gamma_mixture_guide_criterion(end_points, DATASET_CONFIG=None, config=None, *, K=DEFAULT_K, pick=None, sample_inds=None,
                                  return_draws=False, **kwargs):
    """-> (metric_normal, metric_vertical, metric_size, metric_score): 0-dim float32 device tensors, differentiable with
    respect to `last_quad_scores`, `last_quad_center` and `last_quad_size[..., 0]` (the reference detaches everything
    else).  Reads `point_clouds` (B, N, >= 3: the first three columns), `vertex_normals` (B, N, 3) and `last_quad_scores`,
    `last_quad_center`, `last_normal_vector`, `last_quad_size`; writes nothing -- in particular NOT `last_quad_size`, which the
    reference divides by 1.5 in place at [b, pick, 0] (see the module docstring).

    pick (B,) / sample_inds (B, K) (extension): use these draws instead of drawing; with both given no draw is launched
    and the seed counter does not move.  Whether a scene has a candidate quad at all is then derived from the scores.
    return_draws (extension): a fifth value, the dict {pick, skip, sample_inds} of int32 tensors that were used (skip
    is None when both draws were given).  DATASET_CONFIG, config and **kwargs are accepted and unused, as in the reference
    (they only reach its dumping code)."""
    prefix = "last_"
    xyz, normals = end_points["point_clouds"], end_points["vertex_normals"]
    scores, centers = end_points[f"{prefix}quad_scores"], end_points[f"{prefix}quad_center"]
    vectors, sizes = end_points[f"{prefix}normal_vector"], end_points[f"{prefix}quad_size"]
    B, N = xyz.shape[0], xyz.shape[1]
    if sample_inds is not None:
        K = int(sample_inds.shape[1])
    K = int(K)
    if K < 1 or K > MAX_K:
        raise ValueError(f"gamma_mixture_loss_util: K = {K} outside [1, {MAX_K}] (the kept distances of a scene live in LDS)")
    if B == 0:
        zero = torch.zeros((), device=xyz.device, dtype=torch.float32)
        out = (zero, zero.clone(), zero.clone(), zero.clone())
        return out + ({"pick": pick, "skip": None, "sample_inds": sample_inds},) if return_draws else out
    skip = None
    if pick is None or sample_inds is None:
        d_pick, skip, d_inds = draw(scores, N, K)
        if pick is None and sample_inds is None:
            pick, sample_inds = d_pick, d_inds
        else:
            skip = None                          # a caller's pick decides together with the scores, not with our draw
            pick = d_pick if pick is None else pick
            sample_inds = d_inds if sample_inds is None else sample_inds
    pick = _i32(pick, "pick", (B,), xyz)
    sample_inds = _i32(sample_inds, "sample_inds", (B, K), xyz)
    terms, _ = _Guide.apply(scores, centers, sizes, vectors, xyz, normals, pick, skip, sample_inds)
    out = tuple(terms.unbind(0))
    if return_draws:
        return out + ({"pick": pick, "skip": skip, "sample_inds": sample_inds},)
    return out


def scene_records(end_points, pick, sample_inds):
    """(B, RECORD_FLOATS) float32: what the forward leaves per scene (include/omnipq_semi.h) -- the scene's four terms, whether
    it counted, n_k, q85, the kept points' mean, pseudo_x and the score branch.  For tests and diagnostics."""
    xyz = end_points["point_clouds"]
    B = xyz.shape[0]
    pick = _i32(pick, "pick", (B,), xyz)
    sample_inds = _i32(sample_inds, "sample_inds", (B, int(sample_inds.shape[1])), xyz)
    with torch.no_grad():
        _, record = _Guide.apply(end_points["last_quad_scores"], end_points["last_quad_center"], end_points["last_quad_size"],
                                 end_points["last_normal_vector"], xyz, end_points["vertex_normals"], pick, None, sample_inds)
    return record
