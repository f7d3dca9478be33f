// Packed detections (include/omnipq_eval.h): the arithmetic of parse_predictions in front of the suppression
// for every proposal in one launch, and the stable compaction of what the suppression kept into fixed-shape records a graph
// can write and the host can read back in one copy.
// Reference: models/ap_helper_pq.py:73-236 (objects), :323-460 (quads).  Compiled with -ffp-contract=off (build.py): the
// heading is a product and a sum, each rounded on its own.
#include "box_geom.h"
#include "common.h"
#include "omnipq_eval.h"

namespace omnipq {

constexpr int kDetectMaxK = 4096;                // the suppression kernel's limit (eval_ops.hip: kNmsMax)
constexpr int kDetectMaxClasses = 64;            // a proposal's rows are walked by ONE thread
constexpr int kPackThreads = 256;

// first maximum of x[0 .. n); a NaN is larger than every number and the first NaN wins (torch.argmax on the device)
__device__ __forceinline__ int argmax_first(const float *__restrict__ x, int n) {
  float best = x[0];
  int at = 0;
  for (int c = 1; c < n; ++c) {
    const float v = x[c];
    if (best == best && (v > best || v != v)) {
      best = v;
      at = c;
    }
  }
  return at;
}

__global__ __launch_bounds__(256) void decode_boxes_kernel(
    int rows, int nh, int ns, int ncls, const float *__restrict__ center, const float *__restrict__ heading_scores,
    const float *__restrict__ heading_residuals, const float *__restrict__ size_scores,
    const float *__restrict__ size_residuals, const float *__restrict__ sem_cls_scores,
    const float *__restrict__ objectness_scores, const double *__restrict__ mean_size, int heading_rule, int bev,
    int *__restrict__ heading_cls, int *__restrict__ size_cls, int *__restrict__ sem_cls, double *__restrict__ size,
    float *__restrict__ heading, float *__restrict__ obj_prob, float *__restrict__ sem_prob, double *__restrict__ corners8,
    double *__restrict__ aabb) {
  const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= rows) return;
  const size_t rr = (size_t)r;
  const int hc = argmax_first(heading_scores + rr * nh, nh);
  const int sc = argmax_first(size_scores + rr * ns, ns);
  const float *sem = sem_cls_scores + rr * ncls;
  const int cc = argmax_first(sem, ncls);
  heading_cls[r] = hc;
  size_cls[r] = sc;
  sem_cls[r] = cc;

  const float *res = size_residuals + (rr * ns + sc) * 3;
  const double l = mean_size[sc * 3] + (double)res[0];
  const double w = mean_size[sc * 3 + 1] + (double)res[1];
  const double h = mean_size[sc * 3 + 2] + (double)res[2];
  size[rr * 3] = l;
  size[rr * 3 + 1] = w;
  size[rr * 3 + 2] = h;

  float ang = 0.f;
  if (heading_rule) {
    const double two_pi = 6.283185307179586, pi = 3.141592653589793;
    const double per = two_pi / (double)nh;
    const double a = (double)hc * per + (double)heading_residuals[rr * nh + hc];
    ang = (float)(a > pi ? a - two_pi : a);
  }
  heading[r] = ang;

  obj_prob[r] = (float)(1.0 / (1.0 + exp(-(double)objectness_scores[rr * 2 + 1])));

  if (sem_prob) {
    float mx = sem[0];
    for (int c = 1; c < ncls; ++c) mx = sem[c] > mx ? sem[c] : mx;
    double sum = 0.0;
    for (int c = 0; c < ncls; ++c) sum += exp((double)sem[c] - (double)mx);
    for (int c = 0; c < ncls; ++c) sem_prob[rr * ncls + c] = (float)(exp((double)sem[c] - (double)mx) / sum);
  }

  double *box = aabb + rr * 6;
  box_corners_of(ang, l, w, h, center[rr * 3], center[rr * 3 + 1], center[rr * 3 + 2], corners8 + rr * 24, box);
  if (bev) {
    box[1] = 0.0;
    box[4] = 1.0;
  }
}

// One scene, one workgroup of four waves.  Chunks of 256 proposals: every wave ballots its selection, the four wave counts
// cross in LDS, a lane's rank inside the chunk is (counts of the waves before it) + (selected lanes below it), and `running`
// carries the rows written by the chunks before.  The lane that owns a selected proposal writes its scalars; the 192-byte
// corner block and the optional f32 row (class probabilities, F1 corners) of every selected proposal of the chunk are then
// copied by the whole workgroup, element by element, from the source rows listed in LDS.  All pointers are the scene's own;
// cls / ocls, c8 / oc8 and rows / orows are optional pairs.
__device__ __forceinline__ void pack_scene(int k, const unsigned char *__restrict__ keep, const float *__restrict__ score,
                                           float conf, const int *__restrict__ cls, const double *__restrict__ c8,
                                           const float *__restrict__ rows, int rown, int *__restrict__ count,
                                           int *__restrict__ index, int *__restrict__ ocls, float *__restrict__ oscore,
                                           double *__restrict__ oc8, float *__restrict__ orows) {
  __shared__ int src[kPackThreads];
  __shared__ int wave_count[kPackThreads / 64];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int running = 0;
  for (int j0 = 0; j0 < k; j0 += kPackThreads) {
    const int j = j0 + tid;
    const bool sel = j < k && keep[j] != 0 && score[j] > conf;
    const unsigned long long mask = __ballot(sel);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kPackThreads / 64; ++w) {
      const int c = wave_count[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (sel) {
      const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
      const int o = running + pos;                     // < k: at most one row per proposal up to j
      src[pos] = j;
      index[o] = j;
      if (ocls) ocls[o] = cls[j];
      if (oscore) oscore[o] = score[j];
    }
    __syncthreads();
    if (oc8)
      for (int t = tid; t < total * 24; t += kPackThreads) {
        const int row = t / 24, e = t - row * 24;
        oc8[(running + row) * 24 + e] = c8[src[row] * 24 + e];
      }
    if (orows)
      for (int t = tid; t < total * rown; t += kPackThreads) {
        const int row = t / rown, e = t - row * rown;
        orows[(running + row) * rown + e] = rows[src[row] * rown + e];
      }
    running += total;
    __syncthreads();                                   // src and wave_count are rewritten by the next chunk
  }
  for (int j = running + tid; j < k; j += kPackThreads) {
    index[j] = -1;
    if (ocls) ocls[j] = 0;
    if (oscore) oscore[j] = 0.f;
  }
  if (oc8)
    for (int t = running * 24 + tid; t < k * 24; t += kPackThreads) oc8[t] = 0.0;
  if (orows)
    for (int t = running * rown + tid; t < k * rown; t += kPackThreads) orows[t] = 0.f;
  if (tid == 0) *count = running;
}

__global__ __launch_bounds__(kPackThreads) void pack_boxes_kernel(
    int k, int ncls, const unsigned char *__restrict__ keep, const float *__restrict__ score, float conf,
    const int *__restrict__ cls, const double *__restrict__ corners8, const float *__restrict__ sem_prob,
    int *__restrict__ count, int *__restrict__ index, int *__restrict__ out_cls, float *__restrict__ out_score,
    double *__restrict__ out_corners8, float *__restrict__ out_sem_prob) {
  const size_t s = blockIdx.x, sk = s * k;
  pack_scene(k, keep + sk, score + sk, conf, cls + sk, corners8 + sk * 24, sem_prob ? sem_prob + sk * ncls : nullptr, ncls,
             count + s, index + sk, out_cls + sk, out_score + sk, out_corners8 + sk * 24,
             sem_prob ? out_sem_prob + sk * ncls : nullptr);
}

// blockIdx.y: 0 = the AP list (score, corners), 1 = the F1 list (the four corners)
__global__ __launch_bounds__(kPackThreads) void pack_quads_kernel(
    int k, const unsigned char *__restrict__ keep, const float *__restrict__ prob, float conf, float quad_thres,
    const double *__restrict__ corners8, const float *__restrict__ verts4, int *__restrict__ count, int *__restrict__ index,
    float *__restrict__ out_score, double *__restrict__ out_corners8, int *__restrict__ count_f1,
    int *__restrict__ index_f1, float *__restrict__ out_verts4) {
  const size_t s = blockIdx.x, sk = s * k;
  if (blockIdx.y == 0)
    pack_scene(k, keep + sk, prob + sk, conf, nullptr, corners8 + sk * 24, nullptr, 0, count + s, index + sk, nullptr,
               out_score + sk, out_corners8 + sk * 24, nullptr);
  else
    pack_scene(k, keep + sk, prob + sk, quad_thres, nullptr, nullptr, verts4 + sk * 12, 12, count_f1 + s, index_f1 + sk,
               nullptr, nullptr, nullptr, out_verts4 + sk * 12);
}

}  // namespace omnipq

using namespace omnipq;

extern "C" int omnipq_decode_boxes_max_classes(void) { return kDetectMaxClasses; }

static bool classes_ok(int n) { return n >= 1 && n <= kDetectMaxClasses; }

extern "C" int omnipq_decode_boxes(int b, int k, int nh, int ns, int ncls, const float *center, const float *heading_scores,
                                   const float *heading_residuals, const float *size_scores, const float *size_residuals,
                                   const float *sem_cls_scores, const float *objectness_scores, const double *mean_size,
                                   int heading_rule, int bev, int *heading_cls, int *size_cls, int *sem_cls, double *size,
                                   float *heading, float *obj_prob, float *sem_prob, double *corners8, double *aabb,
                                   void *stream) {
  if (b < 0 || k < 0 || k > kDetectMaxK || !classes_ok(nh) || !classes_ok(ns) || !classes_ok(ncls)) return OMNIPQ_EINVAL;
  if (heading_rule != 0 && heading_rule != 1) return OMNIPQ_EINVAL;
  if (b == 0 || k == 0) return OMNIPQ_OK;
  if (!center || !heading_scores || !heading_residuals || !size_scores || !size_residuals || !sem_cls_scores ||
      !objectness_scores || !mean_size || !heading_cls || !size_cls || !sem_cls || !size || !heading || !obj_prob ||
      !corners8 || !aabb)
    return OMNIPQ_EINVAL;
  const long long rows = (long long)b * k;
  if (rows >= (1ll << 31)) return OMNIPQ_EINVAL;
  decode_boxes_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)rows, nh, ns, ncls, center, heading_scores, heading_residuals, size_scores, size_residuals, sem_cls_scores,
      objectness_scores, mean_size, heading_rule, bev != 0, heading_cls, size_cls, sem_cls, size, heading, obj_prob, sem_prob,
      corners8, aabb);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_pack_boxes(int b, int k, int ncls, const unsigned char *keep, const float *score, float conf,
                                 const int *cls, const double *corners8, const float *sem_prob, int *count, int *index,
                                 int *out_cls, float *out_score, double *out_corners8, float *out_sem_prob, void *stream) {
  if (b < 0 || k < 0 || k > kDetectMaxK) return OMNIPQ_EINVAL;
  if ((sem_prob || out_sem_prob) && !classes_ok(ncls)) return OMNIPQ_EINVAL;
  if ((sem_prob == nullptr) != (out_sem_prob == nullptr)) return OMNIPQ_EINVAL;
  if (b == 0 || k == 0) return OMNIPQ_OK;
  if (!keep || !score || !cls || !corners8 || !count || !index || !out_cls || !out_score || !out_corners8)
    return OMNIPQ_EINVAL;
  if (b > 65535) return OMNIPQ_EINVAL;
  pack_boxes_kernel<<<b, kPackThreads, 0, (hipStream_t)stream>>>(k, ncls, keep, score, conf, cls, corners8, sem_prob, count,
                                                                 index, out_cls, out_score, out_corners8, out_sem_prob);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_pack_quads(int b, int k, const unsigned char *keep, const float *prob, float conf, float quad_thres,
                                 const double *corners8, const float *verts4, int *count, int *index, float *out_score,
                                 double *out_corners8, int *count_f1, int *index_f1, float *out_verts4, void *stream) {
  if (b < 0 || k < 0 || k > kDetectMaxK) return OMNIPQ_EINVAL;
  if (b == 0 || k == 0) return OMNIPQ_OK;
  if (!keep || !prob || !corners8 || !verts4 || !count || !index || !out_score || !out_corners8 || !count_f1 || !index_f1 ||
      !out_verts4)
    return OMNIPQ_EINVAL;
  if (b > 65535) return OMNIPQ_EINVAL;
  pack_quads_kernel<<<dim3(b, 2), kPackThreads, 0, (hipStream_t)stream>>>(k, keep, prob, conf, quad_thres, corners8, verts4,
                                                                          count, index, out_score, out_corners8, count_f1,
                                                                          index_f1, out_verts4);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
