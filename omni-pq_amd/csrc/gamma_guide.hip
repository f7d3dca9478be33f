// The gamma-mixture guide criterion (include/omnipq_semi.h; reference models/utils/gamma_mixture_loss_util.py:27-192):
// draw, one workgroup per scene, a reduction over the scenes, one backward launch.  f32 / f64 only: identical in both
// element-type libraries.
#include "common.h"
#include "omnipq_semi.h"
#include "radix_select.h"

namespace omnipq {
namespace {

constexpr int kGmThreads = 512;
constexpr int kGmWaves = kGmThreads / 64;
constexpr int kGmMinKept = 300;                  // :78
constexpr unsigned kInfBits = 0x7f800000u;

// is quad j a candidate (:144): softmax(score)[1] > 0.1, spelled the way torch.softmax computes it
__device__ __forceinline__ bool gm_candidate(const float *score) {
  const float s0 = score[0], s1 = score[1];
  const float m = fmaxf(s0, s1);
  const float e0 = expf(s0 - m), e1 = expf(s1 - m);
  return e1 / (e0 + e1) > 0.1f;
}

// uniform in [0, n) from 32 hashed bits
__device__ __forceinline__ int gm_uniform(unsigned h, int n) { return (int)(((unsigned long long)h * (unsigned)n) >> 32); }

// grid (ceil(k / 256), b).  Every thread one sample index; wave 0 of the scene's first workgroup the pick.
__global__ __launch_bounds__(256) void gm_draw_kernel(int n, int q, int k, const float *__restrict__ quad_scores,
                                                     const unsigned long long *__restrict__ seed, unsigned salt,
                                                     int *__restrict__ pick, int *__restrict__ skip,
                                                     int *__restrict__ sample_inds) {
  const int b = (int)blockIdx.y;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i < k) {
    const unsigned idx = (unsigned)b * (unsigned)k + (unsigned)i;
    sample_inds[(size_t)b * k + i] = gm_uniform(dec_hash(idx, dec_seed(seed, 2u * salt)), n);
  }
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  const int lane = (int)threadIdx.x;
  const float *sc = quad_scores + (size_t)b * q * 2;
  int count = 0;
  for (int j0 = 0; j0 < q; j0 += 64) {
    const int j = j0 + lane;
    const bool c = j < q && gm_candidate(sc + 2 * j);
    count += __popcll(__ballot(c));
  }
  if (count == 0) {
    if (lane == 0) {
      pick[b] = 0;
      skip[b] = 1;
    }
    return;
  }
  int r = gm_uniform(dec_hash((unsigned)b, dec_seed(seed, 2u * salt + 1u)), count);
  for (int j0 = 0; j0 < q; j0 += 64) {
    const int j = j0 + lane;
    const bool c = j < q && gm_candidate(sc + 2 * j);
    unsigned long long mask = __ballot(c);
    const int here = __popcll(mask);
    if (r >= here) {
      r -= here;
      continue;
    }
    for (; r > 0; --r) mask &= mask - 1;          // drop the r lowest candidates of this chunk
    if (lane == 0) {
      pick[b] = j0 + __ffsll((long long)mask) - 1;
      skip[b] = 0;
    }
    return;
  }
}

struct GmQuad {
  float cx, cy, cz, nx, ny, s0, s1, sc0, sc1;
};

// the picked quad of a scene: s0 = s[0] / 1.5 (:29), n = nv.xy / |nv.xy| (:35; 0 / 0 = NaN drops every sample)
__device__ __forceinline__ GmQuad gm_quad(const float *quad_scores, const float *quad_center, const float *normal_vector,
                                          const float *quad_size, size_t row) {
  GmQuad g;
  g.cx = quad_center[3 * row];
  g.cy = quad_center[3 * row + 1];
  g.cz = quad_center[3 * row + 2];
  const float vx = normal_vector[3 * row], vy = normal_vector[3 * row + 1];
  const float nrm = sqrtf(vx * vx + vy * vy);
  g.nx = vx / nrm;
  g.ny = vy / nrm;
  g.s0 = quad_size[2 * row] / 1.5f;
  g.s1 = quad_size[2 * row + 1];
  g.sc0 = quad_scores[2 * row];
  g.sc1 = quad_scores[2 * row + 1];
  return g;
}

struct GmSample {
  bool keep;
  float dn;                                      // o . n (signed); v = |dn|
  float x, y, z, mx, my;
};

// keep <=> weight * dist_a(t) >= (1 - weight) * dist_b(t) with the arguments of :65, as fit.py:170 writes it, in f64
__device__ __forceinline__ bool gm_keep(float total) {
  const double t = fabs((double)total);
  const double lhs = 0.1 * (400.0 / 1.0) * exp(-20.0 * t) * t;
  const double rhs = 0.9 * (1.0 / 2.0) * exp(-t) * (t * t);
  return lhs >= rhs;                              // false for NaN
}

// sample `idx` of the scene against the quad (:34-59).  The forward's two passes and the backward call this same
// function: what one of them keeps, all of them keep.
__device__ __forceinline__ GmSample gm_eval(const GmQuad &g, const float *__restrict__ xyz, int pitch,
                                            const float *__restrict__ normals, int n, int idx) {
  GmSample s;
  s.keep = false;
  s.dn = s.x = s.y = s.z = s.mx = s.my = 0.0f;
  if (idx < 0 || idx >= n) return s;
  const float *p = xyz + (size_t)idx * pitch;
  const float *m = normals + (size_t)idx * 3;
  s.x = p[0];
  s.y = p[1];
  s.z = p[2];
  s.mx = m[0];
  s.my = m[1];
  const float mz = m[2];
  const float mn = fmaxf(sqrtf(s.mx * s.mx + s.my * s.my + mz * mz), 1e-5f);
  const float dc = 1.0f - fabsf(g.nx * (s.mx / mn) + g.ny * (s.my / mn));
  const float ox = s.x - g.cx, oy = s.y - g.cy, oz = s.z - g.cz;
  s.dn = ox * g.nx + oy * g.ny;
  const float xd = fabsf(oy * g.nx - ox * g.ny), zd = fabsf(oz);
  const float a0 = fmaxf(2.0f * xd - g.s0, 0.0f), a1 = fmaxf(2.0f * zd - g.s1, 0.0f);
  const float a = sqrtf(a0 * a0 + a1 * a1);
  const float total = 2.5f * dc + 0.2f * (a * a) + 0.5f * fabsf(s.dn);
  s.keep = gm_keep(total);
  return s;
}

// sum over the workgroup in a fixed order: lanes by shuffles, then the waves' totals one after the other
__device__ __forceinline__ double gm_block_sum(double v, double *scratch) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();                                // scratch may still be read from the previous call
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kGmWaves; ++w) t += scratch[w];
  return t;
}

__device__ __forceinline__ float gm_block_max(float v, double *scratch) {
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_down(v, d, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = (double)v;
  __syncthreads();
  float t = (float)scratch[0];
  for (int w = 1; w < kGmWaves; ++w) t = fmaxf(t, (float)scratch[w]);
  return t;
}

// order statistics and torch.quantile over the workgroup's LDS array: radix_select.h
__device__ __forceinline__ float gm_quantile(const float *vals, int cnt, int n_k, float t, unsigned *hist, unsigned *sel) {
  return radix_quantile<kGmThreads>(vals, cnt, n_k, t, hist, sel);
}

__device__ __forceinline__ double gm_sl1(double e) {
  const double d = fabs(e);
  return d < 1.0 ? 0.5 * d * d : d - 0.5;
}

__device__ __forceinline__ double gm_sl1_grad(double e) {   // abs'(0) = 0, as autograd has it
  const double d = fabs(e);
  const double sgn = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
  return d < 1.0 ? e : sgn;
}

// does the scene take part at all: a pick in range and a candidate quad (skip[] of the draw, or derived the same way)
__device__ bool gm_scene_live(int b, int q, const float *quad_scores, const int *pick, const int *skip, unsigned *sel) {
  const int p = pick[b];
  if (p < 0 || p >= q) return false;
  if (skip) return skip[b] == 0;
  if (threadIdx.x == 0) sel[0] = 0;
  __syncthreads();
  bool any = false;
  for (int j = (int)threadIdx.x; j < q; j += kGmThreads) any |= gm_candidate(quad_scores + ((size_t)b * q + j) * 2);
  if (any) sel[0] = 1;                            // every writer stores the same word
  __syncthreads();
  const bool live = sel[0] != 0;
  __syncthreads();
  return live;
}

__global__ __launch_bounds__(kGmThreads) void gm_guide_kernel(int n, int q, int k, int pitch, const float *__restrict__ xyz,
                                                             const float *__restrict__ normals,
                                                             const float *__restrict__ quad_scores,
                                                             const float *__restrict__ quad_center,
                                                             const float *__restrict__ normal_vector,
                                                             const float *__restrict__ quad_size,
                                                             const int *__restrict__ pick, const int *__restrict__ skip,
                                                             const int *__restrict__ sample_inds, float *__restrict__ record) {
  extern __shared__ float s_vals[];               // k floats
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_sel[4];
  __shared__ double s_red[kGmWaves];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  float *rec = record + (size_t)b * OMNIPQ_GM_RECORD_FLOATS;
  const bool live = gm_scene_live(b, q, quad_scores, pick, skip, s_sel);   // uniform over the workgroup
  if (!live) {
    if (tid < OMNIPQ_GM_RECORD_FLOATS) rec[tid] = 0.0f;
    return;
  }
  const GmQuad g = gm_quad(quad_scores, quad_center, normal_vector, quad_size, (size_t)b * q + pick[b]);
  const float *px = xyz + (size_t)b * n * pitch;
  const float *pm = normals + (size_t)b * n * 3;
  const int *inds = sample_inds + (size_t)b * k;

  // pass 1: keep, the kept vertical distances into LDS, sums of the kept points and of their raw normals
  double cnt = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, smx = 0.0, smy = 0.0;
  for (int i = tid; i < k; i += kGmThreads) {
    const GmSample s = gm_eval(g, px, pitch, pm, n, inds[i]);
    s_vals[i] = s.keep ? fabsf(s.dn) : __uint_as_float(kInfBits);
    if (s.keep) {
      cnt += 1.0;
      sx += (double)s.x;
      sy += (double)s.y;
      sz += (double)s.z;
      smx += (double)s.mx;
      smy += (double)s.my;
    }
  }
  const int n_k = (int)gm_block_sum(cnt, s_red);
  if (n_k < kGmMinKept) {                         // :78, uniform
    if (tid < OMNIPQ_GM_RECORD_FLOATS) rec[tid] = tid == 5 ? (float)n_k : 0.0f;
    return;
  }
  sx = gm_block_sum(sx, s_red);
  sy = gm_block_sum(sy, s_red);
  sz = gm_block_sum(sz, s_red);
  smx = gm_block_sum(smx, s_red);
  smy = gm_block_sum(smy, s_red);
  const float mux = (float)(sx / n_k), muy = (float)(sy / n_k), muz = (float)(sz / n_k);      // :96, an f32 tensor there

  // metric_vertical (:92-93)
  const float q85 = gm_quantile(s_vals, k, n_k, 0.85f, s_hist, s_sel);
  double vs = 0.0;
  for (int i = tid; i < k; i += kGmThreads) {
    const float v = s_vals[i];
    if (v < q85) vs += (double)v;                 // +inf (dropped) is never below a finite q85
  }
  vs = gm_block_sum(vs, s_red);
  const float mv = (float)(vs / n_k);

  // pass 2: |(x - mu) . xdir| of the kept samples (:97-103)
  __syncthreads();
  float top = 0.0f;
  for (int i = tid; i < k; i += kGmThreads) {
    const GmSample s = gm_eval(g, px, pitch, pm, n, inds[i]);
    const float xd = fabsf((s.y - muy) * g.nx - (s.x - mux) * g.ny);
    s_vals[i] = s.keep ? xd : __uint_as_float(kInfBits);
    if (s.keep) top = fmaxf(top, xd);
  }
  top = gm_block_max(top, s_red);                 // quantile(., 1.0): the barriers inside also publish s_vals
  const float x85 = gm_quantile(s_vals, k, n_k, 0.85f, s_hist, s_sel);
  const float x925 = gm_quantile(s_vals, k, n_k, 0.925f, s_hist, s_sel);
  const float pseudo_x = (x85 / 0.85f + x925 / 0.925f + top / 1.0f) / 3.0f;     // :106-112

  if (tid != 0) return;
  // metric_normal (:82-89)
  const double ex = (double)(float)(smx / n_k), ey = (double)(float)(smy / n_k);
  const double en = sqrt(ex * ex + ey * ey);
  const double ux = ex / en, uy = ey / en;
  const double nn = sqrt((double)g.nx * g.nx + (double)g.ny * g.ny), un = sqrt(ux * ux + uy * uy);
  const double cosv = (ux * g.nx + uy * g.ny) / (fmax(un, 1e-8) * fmax(nn, 1e-8));
  const float mnrm = (float)(1.0 - fabs(cosv));
  // metric_size (:114-116)
  const double s0 = (double)quad_size[2 * ((size_t)b * q + pick[b])] / 1.5;
  const double ms_d = gm_sl1(s0 - 2.0 * (double)pseudo_x) + gm_sl1(sx / n_k - g.cx) + gm_sl1(sy / n_k - g.cy) +
                      gm_sl1(sz / n_k - g.cz);
  const float ms = (float)ms_d;
  // metric_score (:119-125)
  int branch = 0;
  if ((double)mv < 0.05 && (double)mnrm < 0.02 && (double)ms < 0.10) branch = 1;
  else if ((double)mv > 0.3 || (double)mnrm > 0.05 || (double)ms > 0.35) branch = 2;
  float msc = 0.0f;
  if (branch) {
    const double m = fmax((double)g.sc0, (double)g.sc1);
    const double lse = m + log(exp((double)g.sc0 - m) + exp((double)g.sc1 - m));
    msc = (float)(lse - (double)(branch == 1 ? g.sc1 : g.sc0));
  }
  rec[0] = mnrm;
  rec[1] = mv;
  rec[2] = ms;
  rec[3] = msc;
  rec[4] = 1.0f;
  rec[5] = (float)n_k;
  rec[6] = q85;
  rec[7] = mux;
  rec[8] = muy;
  rec[9] = muz;
  rec[10] = pseudo_x;
  rec[11] = (float)branch;
}

// terms[t] = sum over the scenes, in scene order, of record[s][t] / b (:185-192)
__global__ __launch_bounds__(64) void gm_terms_kernel(int b, const float *__restrict__ record, float *__restrict__ terms) {
  const int t = (int)threadIdx.x;
  if (t >= 4) return;
  double s = 0.0;
  for (int i = 0; i < b; ++i) s += (double)record[(size_t)i * OMNIPQ_GM_RECORD_FLOATS + t];
  terms[t] = (float)(s / b);
}

__global__ __launch_bounds__(kGmThreads) void gm_guide_grad_kernel(
    int nb, int n, int q, int k, int pitch, const float *__restrict__ xyz, const float *__restrict__ normals,
    const float *__restrict__ quad_scores, const float *__restrict__ quad_center, const float *__restrict__ normal_vector,
    const float *__restrict__ quad_size, const int *__restrict__ pick, const int *__restrict__ sample_inds,
    const float *__restrict__ record, const float *__restrict__ g_terms, float *__restrict__ g_scores,
    float *__restrict__ g_center, float *__restrict__ g_size) {
  __shared__ double s_red[kGmWaves];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const float *rec = record + (size_t)b * OMNIPQ_GM_RECORD_FLOATS;
  const int pk = pick[b];
  const bool valid = rec[4] != 0.0f && pk >= 0 && pk < q;   // the forward only counts a scene whose pick is in range
  const int p = valid ? pk : -1;
  // every row but the picked one: zero
  for (int j = tid; j < q; j += kGmThreads) {
    if (j == p) continue;
    const size_t row = (size_t)b * q + j;
    g_scores[2 * row] = g_scores[2 * row + 1] = 0.0f;
    g_center[3 * row] = g_center[3 * row + 1] = g_center[3 * row + 2] = 0.0f;
    g_size[2 * row] = g_size[2 * row + 1] = 0.0f;
  }
  if (!valid) return;                             // uniform
  const size_t row = (size_t)b * q + p;
  const GmQuad g = gm_quad(quad_scores, quad_center, normal_vector, quad_size, row);
  const float *px = xyz + (size_t)b * n * pitch;
  const float *pm = normals + (size_t)b * n * 3;
  const int *inds = sample_inds + (size_t)b * k;
  const float q85 = rec[6];
  double sgn = 0.0;                               // sum_keep [v < q85] sign(o . n): whole numbers, exact in any order
  for (int i = tid; i < k; i += kGmThreads) {
    const GmSample s = gm_eval(g, px, pitch, pm, n, inds[i]);
    if (s.keep && fabsf(s.dn) < q85) sgn += s.dn > 0.0f ? 1.0 : (s.dn < 0.0f ? -1.0 : 0.0);
  }
  sgn = gm_block_sum(sgn, s_red);
  if (tid != 0) return;
  const double inv_b = 1.0 / nb, n_k = (double)rec[5];
  const double g_mv = (double)g_terms[1] * inv_b, g_ms = (double)g_terms[2] * inv_b, g_sc = (double)g_terms[3] * inv_b;
  const double dv = -g_mv * sgn / n_k;
  g_center[3 * row] = (float)(dv * g.nx - g_ms * gm_sl1_grad((double)rec[7] - g.cx));
  g_center[3 * row + 1] = (float)(dv * g.ny - g_ms * gm_sl1_grad((double)rec[8] - g.cy));
  g_center[3 * row + 2] = (float)(-g_ms * gm_sl1_grad((double)rec[9] - g.cz));
  g_size[2 * row] = (float)(g_ms * gm_sl1_grad((double)g.s0 - 2.0 * (double)rec[10]) / 1.5);
  g_size[2 * row + 1] = 0.0f;
  const int branch = (int)rec[11];
  double d0 = 0.0, d1 = 0.0;
  if (branch) {
    const double m = fmax((double)g.sc0, (double)g.sc1);
    const double e0 = exp((double)g.sc0 - m), e1 = exp((double)g.sc1 - m);
    d0 = e0 / (e0 + e1) - (branch == 2 ? 1.0 : 0.0);
    d1 = e1 / (e0 + e1) - (branch == 1 ? 1.0 : 0.0);
  }
  g_scores[2 * row] = (float)(g_sc * d0);
  g_scores[2 * row + 1] = (float)(g_sc * d1);
}

int gm_check(int b, int n, int q, int k, int pitch) {
  if (b < 0 || n < 1 || q < 1 || k < 1 || pitch < 3) return OMNIPQ_EINVAL;
  if (k > OMNIPQ_GM_MAX_K || (long long)b * k > 0x7fffffffLL || (long long)b * q > 0x7fffffffLL) return OMNIPQ_ETOOLARGE;
  return OMNIPQ_OK;
}

}  // namespace
}  // namespace omnipq

extern "C" int omnipq_gm_draw(int b, int n, int q, int k, const float *quad_scores, const unsigned long long *seed,
                              unsigned salt, int *pick, int *skip, int *sample_inds, void *stream) {
  if (const int rc = omnipq::gm_check(b, n, q, k, 3)) return rc;
  if (b > 65535) return OMNIPQ_ETOOLARGE;         // scenes ride on grid.y
  if (b == 0) return OMNIPQ_OK;
  if (!quad_scores || !seed || !pick || !skip || !sample_inds) return OMNIPQ_EINVAL;
  omnipq::gm_draw_kernel<<<dim3((unsigned)((k + 255) / 256), (unsigned)b), 256, 0, (hipStream_t)stream>>>(
      n, q, k, quad_scores, seed, salt, pick, skip, sample_inds);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_gm_guide(int b, int n, int q, int k, int xyz_pitch, const float *xyz, const float *normals,
                               const float *quad_scores, const float *quad_center, const float *normal_vector,
                               const float *quad_size, const int *pick, const int *skip, const int *sample_inds,
                               float *record, float *terms, void *stream) {
  if (const int rc = omnipq::gm_check(b, n, q, k, xyz_pitch)) return rc;
  if (b == 0) return OMNIPQ_OK;
  if (!xyz || !normals || !quad_scores || !quad_center || !normal_vector || !quad_size || !pick || !sample_inds || !record ||
      !terms)
    return OMNIPQ_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  omnipq::gm_guide_kernel<<<(unsigned)b, omnipq::kGmThreads, (size_t)k * sizeof(float), st>>>(
      n, q, k, xyz_pitch, xyz, normals, quad_scores, quad_center, normal_vector, quad_size, pick, skip, sample_inds, record);
  OMNIPQ_LAUNCH_CHECK();
  omnipq::gm_terms_kernel<<<1, 64, 0, st>>>(b, record, terms);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_gm_guide_grad(int b, int n, int q, int k, int xyz_pitch, const float *xyz, const float *normals,
                                    const float *quad_scores, const float *quad_center, const float *normal_vector,
                                    const float *quad_size, const int *pick, const int *sample_inds, const float *record,
                                    const float *g_terms, float *g_quad_scores, float *g_quad_center, float *g_quad_size,
                                    void *stream) {
  if (const int rc = omnipq::gm_check(b, n, q, k, xyz_pitch)) return rc;
  if (b == 0) return OMNIPQ_OK;
  if (!xyz || !normals || !quad_scores || !quad_center || !normal_vector || !quad_size || !pick || !sample_inds || !record ||
      !g_terms || !g_quad_scores || !g_quad_center || !g_quad_size)
    return OMNIPQ_EINVAL;
  omnipq::gm_guide_grad_kernel<<<(unsigned)b, omnipq::kGmThreads, 0, (hipStream_t)stream>>>(
      b, n, q, k, xyz_pitch, xyz, normals, quad_scores, quad_center, normal_vector, quad_size, pick, sample_inds, record,
      g_terms, g_quad_scores, g_quad_center, g_quad_size);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
