// Oriented-box IoU of the detection metrics (include/omnipq_eval.h: omnipq_obb_iou_pairs, omnipq_obb_iou_best).
// Restates omni-pq_amd/eval_det.py: box3d_iou / _clip / _shoelace / _volume operation for operation in f64 (this file is
// compiled with -ffp-contract=off: every product is rounded before it is added, as Python does), so every `inside`
// decision of the clipping is the host's.  Only the order in which the shoelace sums add their terms differs from
// numpy's dot.
//
// Layout: one thread per pair / per detection.  The clipped polygon's vertices need runtime-indexed storage, which would
// go to scratch as a private array; each thread owns a slice of LDS instead, laid out [coordinate of a vertex][thread], so
// the 64 lanes of a wave read and write 64 consecutive doubles.
// The arithmetic itself -- what one thread computes -- is csrc/obb_iou.h, which also compiles as host C++.
#include "common.h"
#include "obb_iou.h"
#include "omnipq_eval.h"

namespace omnipq {

__global__ __launch_bounds__(kIouThreads) void obb_iou_pairs_kernel(long long n, const double *__restrict__ a8,
                                                                    const double *__restrict__ b8,
                                                                    double *__restrict__ iou3d,
                                                                    double *__restrict__ iou2d) {
  __shared__ double verts[kIouRows * kIouThreads];
  const long long i = (long long)blockIdx.x * kIouThreads + threadIdx.x;
  if (i >= n) return;
  const ObbBox a = load_box(a8 + i * 24), b = load_box(b8 + i * 24);
  double v3, v2;
  obb_iou(a, b, verts + threadIdx.x, v3, v2);
  if (iou3d) iou3d[i] = v3;
  if (iou2d) iou2d[i] = v2;
}

// eval_det_cls's inner loop for detection i: over the ground truth of its segment in order, replace on a strict `>`
__global__ __launch_bounds__(kIouThreads) void obb_iou_best_kernel(long long n_pred, const double *__restrict__ pred8,
                                                                   const int *__restrict__ pred_seg, int n_seg,
                                                                   const long long *__restrict__ seg_start, long long n_gt,
                                                                   const double *__restrict__ gt8,
                                                                   double *__restrict__ ovmax, int *__restrict__ jmax) {
  __shared__ double verts[kIouRows * kIouThreads];
  const long long i = (long long)blockIdx.x * kIouThreads + threadIdx.x;
  if (i >= n_pred) return;
  double best = -INFINITY;
  int jbest = -1;
  const int s = pred_seg[i];
  if (s >= 0 && s < n_seg) {                                    // a segment id outside the table reads nothing
    long long j0 = seg_start[s], j1 = seg_start[s + 1];
    j0 = j0 < 0 ? 0 : j0;
    j1 = j1 > n_gt ? n_gt : j1;                                 // ... and neither does a table that points past gt8
    if (j0 < j1) {
      const ObbBox p = load_box(pred8 + i * 24);
      for (long long j = j0; j < j1; ++j) {
        const ObbBox g = load_box(gt8 + j * 24);
        double v3, v2;
        obb_iou(p, g, verts + threadIdx.x, v3, v2);
        if (v3 > best) {                                        // false for a NaN overlap: it never wins
          best = v3;
          jbest = (int)(j - j0);
        }
      }
    }
  }
  ovmax[i] = best;
  jmax[i] = jbest;
}

}  // namespace omnipq

using namespace omnipq;

extern "C" int omnipq_obb_iou_pairs(long long n, const double *a8, const double *b8, double *iou3d, double *iou2d,
                                    void *stream) {
  if (n < 0) return OMNIPQ_EINVAL;
  if (n == 0) return OMNIPQ_OK;
  if (!a8 || !b8 || (!iou3d && !iou2d)) return OMNIPQ_EINVAL;
  if (n >= (1ll << 31)) return OMNIPQ_ETOOLARGE;
  obb_iou_pairs_kernel<<<(unsigned)((n + kIouThreads - 1) / kIouThreads), kIouThreads, 0, (hipStream_t)stream>>>(
      n, a8, b8, iou3d, iou2d);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_obb_iou_best(long long n_pred, const double *pred8, const int *pred_seg, int n_seg,
                                   const long long *seg_start, long long n_gt, const double *gt8, double *ovmax, int *jmax,
                                   void *stream) {
  if (n_pred < 0 || n_gt < 0 || n_seg < 0) return OMNIPQ_EINVAL;
  if (n_pred == 0) return OMNIPQ_OK;
  if (n_seg <= 0) return OMNIPQ_EINVAL;
  if (!pred8 || !pred_seg || !seg_start || !ovmax || !jmax || (n_gt > 0 && !gt8)) return OMNIPQ_EINVAL;
  if (n_pred >= (1ll << 31) || n_gt >= (1ll << 31)) return OMNIPQ_ETOOLARGE;
  obb_iou_best_kernel<<<(unsigned)((n_pred + kIouThreads - 1) / kIouThreads), kIouThreads, 0, (hipStream_t)stream>>>(
      n_pred, pred8, pred_seg, n_seg, seg_start, n_gt, gt8, ovmax, jmax);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
