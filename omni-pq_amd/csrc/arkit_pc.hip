// The ARKit physical-constraint loss (include/omnipq_semi.h; reference models/utils/arkit_loss_util.py:5-52 with
// models/loss_helper_pq.py:307-350 `get_2d_box` / `projection2d`): the footprint corners of an unlabelled scene's ground-truth
// boxes against every predicted quad whose score passes 0.1.  One workgroup per scene (the scene's boxes in LDS, one thread
// per quad looping over the corners), a one-wave fold over the scenes; one backward launch.  f32 inputs, f64 arithmetic per
// pair: identical in both element-type libraries.  The backward takes the forward's decisions by evaluating the SAME
// functions (ark_quad, ark_pair) on the same inputs; the build compiles without FP contraction, so they give the same bits.
#include "common.h"
#include "omnipq_semi.h"

namespace omnipq {
namespace {

constexpr int kArkThreads = 256;
constexpr int kArkWaves = kArkThreads / 64;
constexpr double kArkGate = 0.1;                 // arkit_loss_util.py:45
constexpr double kArkHit = 1e-4;                 // loss_helper_pq.py:349

struct ArkQuad {
  double a, b, cx, cy, d0, size0;                // (a, b): the normal turned inwards; d0 = a cx + b cy
  int gate, rev;
};

__device__ __forceinline__ ArkQuad ark_quad(const float *__restrict__ quad_center, const float *__restrict__ normal_vector,
                                            const float *__restrict__ quad_size, const float *__restrict__ quad_scores,
                                            size_t row) {
  ArkQuad g;
  const double s0 = (double)quad_scores[2 * row], s1 = (double)quad_scores[2 * row + 1];
  g.gate = 1.0 / (1.0 + exp(s0 - s1)) > kArkGate ? 1 : 0;       // softmax(.)[1]; NaN scores do not pass
  g.cx = (double)quad_center[3 * row];
  g.cy = (double)quad_center[3 * row + 1];
  const double nx = (double)normal_vector[3 * row], ny = (double)normal_vector[3 * row + 1];
  g.rev = -(g.cx * nx + g.cy * ny) < 0.0 ? 1 : 0;               // (pseudo scene centre - c) . n with z dropped (:35-38)
  g.a = g.rev ? -nx : nx;
  g.b = g.rev ? -ny : ny;
  g.d0 = g.a * g.cx + g.b * g.cy;
  g.size0 = (double)quad_size[2 * row];
  return g;
}

// one corner against one quad: delta, and whether the corner's projection lies within size0 of the quad's centre
__device__ __forceinline__ bool ark_pair(const ArkQuad &g, double px, double py, double &delta) {
  delta = (g.a * px + g.b * py) - g.d0;
  const double ex = (px - g.a * delta) - g.cx, ey = (py - g.b * delta) - g.cy;
  return sqrt(ex * ex + ey * ey) < g.size0;
}

// corner c of a box (gx, gy, l, w): (+, +), (+, -), (-, +), (-, -) as get_2d_box lays them out
__device__ __forceinline__ void ark_corner(const float4 &box, int c, double &px, double &py) {
  const double hl = 0.5 * (double)box.z, hw = 0.5 * (double)box.w;
  px = (double)box.x + (c < 2 ? hl : -hl);
  py = (double)box.y + ((c & 1) ? -hw : hw);
}

// the first min(n_s, k2) boxes of scene s -> LDS; rows beyond are never read.  Returns that number.
__device__ __forceinline__ int ark_load_boxes(int s, int k2, const float *__restrict__ center_label,
                                              const float *__restrict__ size_label, long long n_s, float4 *s_box) {
  const int nb = n_s < 0 ? 0 : (n_s < (long long)k2 ? (int)n_s : k2);
  for (int i = (int)threadIdx.x; i < nb; i += kArkThreads) {
    const size_t r = ((size_t)s * k2 + i) * 3;
    s_box[i] = make_float4(center_label[r], center_label[r + 1], size_label[r], size_label[r + 1]);
  }
  __syncthreads();
  return nb;
}

// sum over the workgroup in a fixed order: lanes by shuffles, then the waves' totals one after the other
__device__ __forceinline__ double ark_block_sum(double v, double *scratch) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();                                // scratch may still be read from the previous call
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kArkWaves; ++w) t += scratch[w];
  return t;
}

// grid (b): scene_sums[2 s] = the scene's loss, [2 s + 1] = its collisions
__global__ __launch_bounds__(kArkThreads) void ark_fwd_kernel(
    int first, int q, int k2, const float *__restrict__ quad_center, const float *__restrict__ normal_vector,
    const float *__restrict__ quad_size, const float *__restrict__ quad_scores, const float *__restrict__ center_label,
    const float *__restrict__ size_label, const long long *__restrict__ num_gt_boxes, long long count_stride,
    int *__restrict__ record, double *__restrict__ scene_sums) {
  __shared__ float4 s_box[OMNIPQ_ARKIT_MAX_BOXES];
  __shared__ double s_red[kArkWaves];
  const int s = (int)blockIdx.x;
  const long long n_s = num_gt_boxes[(size_t)s * (size_t)count_stride];
  const int nb = ark_load_boxes(s, k2, center_label, size_label, n_s, s_box);
  double loss = 0.0, hits = 0.0;
  for (int j = (int)threadIdx.x; j < q; j += kArkThreads) {
    const ArkQuad g = ark_quad(quad_center, normal_vector, quad_size, quad_scores, (size_t)(first + s) * q + j);
    int inside = 0, live = 0, hit = 0;
    if (g.gate) {
      double sum = 0.0;
      for (int i = 0; i < nb; ++i) {
        const float4 box = s_box[i];
        for (int c = 0; c < 4; ++c) {
          double px, py, delta;
          ark_corner(box, c, px, py);
          if (!ark_pair(g, px, py, delta)) continue;
          ++inside;
          if (delta < 0.0) {                      // relu(-delta), relu'(0) = 0
            ++live;
            sum += -delta;
            hit += -delta > kArkHit ? 1 : 0;
          }
        }
      }
      if (nb > 0) loss += sum / (double)n_s;      // n_s = 0: the scene contributes nothing (the reference: 0 / 0)
      hits += (double)hit;
    }
    int *rec = record + ((size_t)s * q + j) * OMNIPQ_ARKIT_RECORD_INTS;
    rec[0] = g.gate;
    rec[1] = g.gate ? g.rev : 0;                  // decided for the quads that count only
    rec[2] = inside;
    rec[3] = live;
    rec[4] = hit;
  }
  loss = ark_block_sum(loss, s_red);
  hits = ark_block_sum(hits, s_red);
  if (threadIdx.x == 0) {
    scene_sums[2 * s] = loss;
    scene_sums[2 * s + 1] = hits;
  }
}

// out[t] = sum over the scenes, in scene order (no division by the batch size: arkit_loss_util.py:49)
__global__ __launch_bounds__(64) void ark_fold_kernel(int b, const double *__restrict__ scene_sums, float *__restrict__ out) {
  const int t = (int)threadIdx.x;
  if (t >= 2) return;
  double s = 0.0;
  for (int i = 0; i < b; ++i) s += scene_sums[2 * i + t];
  out[t] = (float)s;
}

// grid (first + b): the labelled scenes' rows are zeroed, every other row is written once.  On a live pair the term is
// -delta = -(a (px - cx) + b (py - cy)):  d / da = -(px - cx), d / db = -(py - cy), d / dcx = a, d / dcy = b, and
// (a, b) = sgn (nx, ny) with sgn = -1 for a reversed normal (no gradient through the reversal itself: the centre is detached).
__global__ __launch_bounds__(kArkThreads) void ark_grad_kernel(
    int first, int q, int k2, const float *__restrict__ quad_center, const float *__restrict__ normal_vector,
    const float *__restrict__ quad_size, const float *__restrict__ quad_scores, const float *__restrict__ center_label,
    const float *__restrict__ size_label, const long long *__restrict__ num_gt_boxes, long long count_stride,
    const int *__restrict__ record, const float *__restrict__ g_out, float *__restrict__ g_quad_center,
    float *__restrict__ g_normal_vector) {
  __shared__ float4 s_box[OMNIPQ_ARKIT_MAX_BOXES];
  const int scene = (int)blockIdx.x;
  if (scene < first) {                            // uniform over the block
    for (int j = (int)threadIdx.x; j < q; j += kArkThreads) {
      const size_t o = ((size_t)scene * q + j) * 3;
      g_quad_center[o] = g_quad_center[o + 1] = g_quad_center[o + 2] = 0.0f;
      g_normal_vector[o] = g_normal_vector[o + 1] = g_normal_vector[o + 2] = 0.0f;
    }
    return;
  }
  const int s = scene - first;
  const long long n_s = num_gt_boxes[(size_t)s * (size_t)count_stride];
  const int nb = ark_load_boxes(s, k2, center_label, size_label, n_s, s_box);
  const double go = (double)g_out[0];
  for (int j = (int)threadIdx.x; j < q; j += kArkThreads) {
    const size_t row = (size_t)scene * q + j;
    const int *rec = record + ((size_t)s * q + j) * OMNIPQ_ARKIT_RECORD_INTS;
    double gcx = 0.0, gcy = 0.0, gnx = 0.0, gny = 0.0;
    if (rec[0] != 0 && rec[3] > 0 && nb > 0) {    // the forward found live pairs here
      const ArkQuad g = ark_quad(quad_center, normal_vector, quad_size, quad_scores, row);
      double sx = 0.0, sy = 0.0;
      int live = 0;
      for (int i = 0; i < nb; ++i) {
        const float4 box = s_box[i];
        for (int c = 0; c < 4; ++c) {
          double px, py, delta;
          ark_corner(box, c, px, py);
          if (ark_pair(g, px, py, delta) && delta < 0.0) {
            sx += px - g.cx;
            sy += py - g.cy;
            ++live;
          }
        }
      }
      const double scale = go / (double)n_s, sgn = g.rev ? -1.0 : 1.0;
      gnx = -(scale * sgn) * sx;
      gny = -(scale * sgn) * sy;
      gcx = scale * (double)live * g.a;
      gcy = scale * (double)live * g.b;
    }
    g_quad_center[3 * row] = (float)gcx;
    g_quad_center[3 * row + 1] = (float)gcy;
    g_quad_center[3 * row + 2] = 0.0f;
    g_normal_vector[3 * row] = (float)gnx;
    g_normal_vector[3 * row + 1] = (float)gny;
    g_normal_vector[3 * row + 2] = 0.0f;
  }
}

int ark_check(int first, int b, int q, int k2, long long count_stride) {
  if (b < 0 || first < 0 || q < 1 || k2 < 1 || count_stride < 1) return OMNIPQ_EINVAL;
  if (k2 > OMNIPQ_ARKIT_MAX_BOXES) return OMNIPQ_ETOOLARGE;
  // row and record offsets are computed in size_t; the grid and the int loop counters bound the rest
  if (((long long)first + b) * q > 0x7fffffffLL / OMNIPQ_ARKIT_RECORD_INTS || (long long)first + b > 0x7fffffffLL)
    return OMNIPQ_ETOOLARGE;
  return OMNIPQ_OK;
}

}  // namespace
}  // namespace omnipq

extern "C" int omnipq_arkit_pc(int first, int b, int q, int k2, const float *quad_center, const float *normal_vector,
                               const float *quad_size, const float *quad_scores, const float *center_label,
                               const float *size_label, const long long *num_gt_boxes, long long count_stride, int *record,
                               double *scene_sums, float *out, void *stream) {
  if (const int rc = omnipq::ark_check(first, b, q, k2, count_stride)) return rc;
  if (b == 0) return OMNIPQ_OK;
  if (!quad_center || !normal_vector || !quad_size || !quad_scores || !center_label || !size_label || !num_gt_boxes ||
      !record || !scene_sums || !out)
    return OMNIPQ_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  omnipq::ark_fwd_kernel<<<(unsigned)b, omnipq::kArkThreads, 0, st>>>(first, q, k2, quad_center, normal_vector, quad_size,
                                                                     quad_scores, center_label, size_label, num_gt_boxes,
                                                                     count_stride, record, scene_sums);
  OMNIPQ_LAUNCH_CHECK();
  omnipq::ark_fold_kernel<<<1, 64, 0, st>>>(b, scene_sums, out);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_arkit_pc_grad(int first, int b, int q, int k2, const float *quad_center, const float *normal_vector,
                                    const float *quad_size, const float *quad_scores, const float *center_label,
                                    const float *size_label, const long long *num_gt_boxes, long long count_stride,
                                    const int *record, const float *g_out, float *g_quad_center, float *g_normal_vector,
                                    void *stream) {
  if (const int rc = omnipq::ark_check(first, b, q, k2, count_stride)) return rc;
  if (b == 0) return OMNIPQ_OK;
  if (!quad_center || !normal_vector || !quad_size || !quad_scores || !center_label || !size_label || !num_gt_boxes ||
      !record || !g_out || !g_quad_center || !g_normal_vector)
    return OMNIPQ_EINVAL;
  omnipq::ark_grad_kernel<<<(unsigned)(first + b), omnipq::kArkThreads, 0, (hipStream_t)stream>>>(
      first, q, k2, quad_center, normal_vector, quad_size, quad_scores, center_label, size_label, num_gt_boxes, count_stride,
      record, g_out, g_quad_center, g_normal_vector);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
