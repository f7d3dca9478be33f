// Layout F1 on the device (include/omnipq_eval.h): the counts of QUADAPCalculator.compute_F1 for a batch in one
// launch, added to an integer accumulator the host reads once per epoch.
// Reference: models/ap_helper_pq.py:647-736 (same_point, compute_correctness, get_ceiling_and_floor, compute_F1).
// Compiled with -ffp-contract=off (build.py): a distance is three f64 products and two sums, each rounded on its own, as
// numpy forms it; a fused step could move a corner across the threshold.
#include "common.h"
#include "omnipq_eval.h"

namespace omnipq {

constexpr int kF1MaxK = 4096;                    // the quad record's limit (detect.hip: kDetectMaxK)
constexpr int kF1Threads = 256;
constexpr int kF1MaxGt = kF1Threads;             // the ground-truth rows are staged by one thread each
constexpr int kF1MaxH = 8;

// sqrt((dx dx + dy dy) + dz dz) <= thr with both corners widened to f64; a NaN never passes
__device__ __forceinline__ bool f1_near(const float *__restrict__ a, const float *__restrict__ b, double thr) {
  const double dx = (double)a[0] - (double)b[0];
  const double dy = (double)a[1] - (double)b[1];
  const double dz = (double)a[2] - (double)b[2];
  return sqrt((dx * dx + dy * dy) + dz * dz) <= thr;
}

// is the quad p (4 x 3) within thr of some quad of list (n x 4 x 3), corner by corner, in the same order or with the two
// corners of each edge swapped ([1, 0, 3, 2])?  Leaves at the first quad that matches.
__device__ __forceinline__ bool f1_correct(const float *__restrict__ p, const float *__restrict__ list, int n, double thr) {
  for (int q = 0; q < n; ++q) {
    const float *G = list + q * 12;
    bool same = true, swapped = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      same = same && f1_near(p + i * 3, G + i * 3, thr);
      swapped = swapped && f1_near(p + i * 3, G + (i ^ 1) * 3, thr);
    }
    if (same || swapped) return true;
  }
  return false;
}

// One scene, one workgroup of four waves.  The scene's ground-truth list (rows j < num_total[s, min(j, cols - 1)], compacted
// in increasing j by ballot ranks) and its horizontal rows are staged in LDS; then one thread per predicted quad and chunk of
// 256, its twelve floats in registers; every wave counts its correct quads by ballot and the four counts cross in LDS.
// Thread 0 finishes: the ceiling and floor of a two-quad scene, the per_scene row, the integer atomics.
__global__ __launch_bounds__(kF1Threads) void layout_f1_kernel(
    int k, const int *__restrict__ count_f1, const float *__restrict__ verts4, int g, const float *__restrict__ gt_verts4,
    const long long *__restrict__ num_total, int cols, int h, const float *__restrict__ horizontal, double thr,
    int *__restrict__ per_scene, unsigned long long *__restrict__ acc) {
  __shared__ float gt[kF1MaxGt * 12];
  __shared__ float hz[kF1MaxH * 12];
  __shared__ int wave_count[kF1Threads / 64];
  const size_t s = blockIdx.x;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;

  // ---- the ground-truth list (g <= kF1MaxGt: one row per thread) and the horizontal rows
  bool listed = false;
  if (tid < g) {
    const int col = tid < cols - 1 ? tid : cols - 1;
    listed = (long long)tid < num_total[s * cols + col];
  }
  const unsigned long long mask = __ballot(listed);
  if (lane == 0) wave_count[wave] = __popcll(mask);
  for (int t = tid; t < h * 12; t += kF1Threads) hz[t] = horizontal[s * h * 12 + t];
  __syncthreads();
  int before = 0, npos = 0;
#pragma unroll
  for (int w = 0; w < kF1Threads / 64; ++w) {
    const int c = wave_count[w];
    before += w < wave ? c : 0;
    npos += c;
  }
  if (listed) {
    const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));       // < g
    const float *src = gt_verts4 + (s * g + tid) * 12;
#pragma unroll
    for (int e = 0; e < 12; ++e) gt[pos * 12 + e] = src[e];
  }
  __syncthreads();                                   // gt is complete; wave_count has been read by everyone

  // ---- the predicted quads
  int n = count_f1[s];
  n = n < 0 ? 0 : (n > k ? k : n);
  const float *quads = verts4 + s * k * 12;
  int tp_wave = 0;
  for (int j0 = 0; j0 < n; j0 += kF1Threads) {
    const int j = j0 + tid;
    bool correct = false;
    if (j < n) {
      float p[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) p[e] = quads[(size_t)j * 12 + e];
      correct = f1_correct(p, gt, npos, thr);
    }
    tp_wave += __popcll(__ballot(correct));
  }
  if (lane == 0) wave_count[wave] = tp_wave;
  __syncthreads();
  if (tid != 0) return;
  int tp = 0;
#pragma unroll
  for (int w = 0; w < kF1Threads / 64; ++w) tp += wave_count[w];

  // ---- ceiling (corners 0, 1) and floor (corners 2, 3) deduced from the walls of a two-quad scene
  int tp_h = 0;
  if (n == 2) {
    for (int side = 0; side < 2; ++side) {
      float e[12];
#pragma unroll
      for (int c = 0; c < 4; ++c) {                  // corner `side * 2 + (c & 1)` of quad c >> 1
        const float *q = quads + (c >> 1) * 12 + (side * 2 + (c & 1)) * 3;
        float x = q[0], y = q[1], z = q[2];
        const float cur[3] = {x, y, z};
        bool merged = false;
#pragma unroll
        for (int f = 0; f < c; ++f)
          if (!merged && f1_near(e + f * 3, cur, thr)) {                     // the FIRST entry within reach
            merged = true;
            x = (e[f * 3] + x) * 0.5f;               // the f32 midpoint: the sum is rounded, the halving is exact
            y = (e[f * 3 + 1] + y) * 0.5f;
            z = (e[f * 3 + 2] + z) * 0.5f;
          }
        e[c * 3] = x;
        e[c * 3 + 1] = y;
        e[c * 3 + 2] = z;
      }
      tp_h += f1_correct(e, hz, h, thr) ? 1 : 0;     // against ALL h rows, the zero padding rows included
    }
  }

  const int fp = n - tp;
  if (per_scene) {
    per_scene[s * 4] = tp;
    per_scene[s * 4 + 1] = fp;
    per_scene[s * 4 + 2] = npos;
    per_scene[s * 4 + 3] = tp_h;
  }
  if (acc) {
    atomicAdd(acc, (unsigned long long)tp);
    atomicAdd(acc + 1, (unsigned long long)fp);
    atomicAdd(acc + 2, (unsigned long long)npos);
    atomicAdd(acc + 3, (unsigned long long)tp_h);
    atomicAdd(acc + 4, 1ull);
  }
}

}  // namespace omnipq

using namespace omnipq;

extern "C" int omnipq_layout_f1_max_gt(void) { return kF1MaxGt; }

extern "C" int omnipq_layout_f1(int b, int k, const int *count_f1, const float *verts4, int g, const float *gt_verts4,
                                const long long *num_total, int num_total_cols, int h, const float *horizontal,
                                double same_thres, int *per_scene, long long *acc, void *stream) {
  if (b < 0 || k < 0 || k > kF1MaxK || g < 0 || g > kF1MaxGt || h < 0 || h > kF1MaxH || num_total_cols < 1)
    return OMNIPQ_EINVAL;
  if (!(same_thres >= 0.0) || same_thres > 1.7976931348623157e308) return OMNIPQ_EINVAL;      // NaN, negative, infinite
  if (b == 0) return OMNIPQ_OK;
  if (!per_scene && !acc) return OMNIPQ_EINVAL;
  if (!count_f1 || (k > 0 && !verts4) || (g > 0 && (!gt_verts4 || !num_total)) || (h > 0 && !horizontal))
    return OMNIPQ_EINVAL;
  layout_f1_kernel<<<b, kF1Threads, 0, (hipStream_t)stream>>>(k, count_f1, verts4, g, gt_verts4, num_total, num_total_cols, h,
                                                              horizontal, same_thres, per_scene,
                                                              (unsigned long long *)acc);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
