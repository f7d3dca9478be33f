// The mean-teacher consistency loss (include/omnipq_semi.h; reference models/utils/mean_teacher_consistency_util.py:21-270):
// rows (one workgroup per scene, prefix and kind), clip (one workgroup per prefix and kind), a one-wave fold; one backward
// launch.  f32 inputs, f64 arithmetic per row: identical in both element-type libraries.
#include "common.h"
#include "omnipq_semi.h"
#include "radix_select.h"

namespace omnipq {
namespace {

constexpr int kMtThreads = 512;
constexpr int kMtWaves = kMtThreads / 64;
constexpr float kMtClip = 0.85f;                 // EMA_CLIP (:17)
constexpr double kMtCosEps = 1e-8;               // F.cosine_similarity's eps

// byte offsets into the workspace; pk = 2 * prefix + kind, n = b * k
struct MtLayout {
  long long kl;                                  // double [2 prefixes][b]: the scene's KL sum
  long long rec;                                 // double [2 prefixes][4]: masked sums of the three arrays, KL sum
  long long vals;                                // float  [2 prefixes][3][n]: d; size | normal; - | quad size
  long long ind1, ind2;                          // int    [2 prefixes][n]
  long long cls;                                 // int    [prefixes][2][n]: arg-max size class, student's | teacher's
  long long eps;                                 // float  [2 prefixes][4]
  long long mask;                                // uchar  [2 prefixes][3][n]
  long long bytes;
};

__host__ __device__ inline MtLayout mt_layout(int prefixes, int b, int k) {
  const long long n = (long long)b * k, pk = 2LL * prefixes;
  MtLayout l;
  long long o = 0;
  l.kl = o, o += pk * b * 8;
  l.rec = o, o += pk * 4 * 8;
  l.vals = o, o += pk * 3 * n * 4;
  l.ind1 = o, o += pk * n * 4;
  l.ind2 = o, o += pk * n * 4;
  l.cls = o, o += pk * n * 4;
  l.eps = o, o += pk * 4 * 4;
  l.mask = o, o += pk * 3 * n;
  l.bytes = (o + 255) & ~255LL;
  return l;
}

struct MtWs {
  double *kl, *rec;
  float *vals, *eps;
  int *ind1, *ind2, *cls;
  unsigned char *mask;
};

__device__ __forceinline__ MtWs mt_ws(void *base, int prefixes, int b, int k) {
  const MtLayout l = mt_layout(prefixes, b, k);
  unsigned char *p = (unsigned char *)base;
  MtWs w;
  w.kl = (double *)(p + l.kl);
  w.rec = (double *)(p + l.rec);
  w.vals = (float *)(p + l.vals);
  w.ind1 = (int *)(p + l.ind1);
  w.ind2 = (int *)(p + l.ind2);
  w.cls = (int *)(p + l.cls);
  w.eps = (float *)(p + l.eps);
  w.mask = p + l.mask;
  return w;
}

// one scene of one prefix and kind in LDS: 68 bytes per proposal
struct MtScene {
  double *e, *s, *d1, *d2;                       // aligned teacher centres (k, 3), confidences, dist1, dist2
  float *c;                                      // student centres (k, 3)
  int *i1, *i2;
};

__device__ __forceinline__ MtScene mt_scene(unsigned char *base, int k) {
  MtScene m;
  m.e = (double *)base;
  m.s = m.e + 3 * k;
  m.d1 = m.s + k;
  m.d2 = m.d1 + k;
  m.c = (float *)(m.d2 + k);
  m.i1 = (int *)(m.c + 3 * k);
  m.i2 = m.i1 + k;
  return m;
}

constexpr int kMtSceneBytes = 68;

__device__ __forceinline__ double mt_sq3(const float *c, const double *e) {
  const double dx = (double)c[0] - e[0], dy = (double)c[1] - e[1], dz = (double)c[2] - e[2];
  return dx * dx + dy * dy + dz * dz;
}

// softmax(score)[1]
__device__ __forceinline__ double mt_conf(const float *score) {
  const double s0 = (double)score[0], s1 = (double)score[1];
  const double m = fmax(s0, s1);
  const double e0 = exp(s0 - m), e1 = exp(s1 - m);
  return e1 / (e0 + e1);
}

// the student's centres, the teacher's centres aligned with them (:30-39) and the student's confidences (:42) of scene b
__device__ void mt_stage(const omnipq_mt_desc &d, int b, int p, int quad, const MtScene &m) {
  const int k = d.k;
  const size_t row0 = (size_t)b * k;
  const float *cs = (quad ? d.quad_center[p] : d.center[p]) + row0 * 3;
  const float *ct = (quad ? d.t_quad_center[p] : d.t_center[p]) + row0 * 3;
  const float *sc = (quad ? d.quad_scores[p] : d.objectness_scores[p]) + row0 * 2;
  const double fx = d.flip_x[b] != 0 ? -1.0 : 1.0, fy = d.flip_y[b] != 0 ? -1.0 : 1.0;
  const float *rot = d.rot_mat + (size_t)b * 9;
  const double scale = (double)d.scale[b];
  for (int i = (int)threadIdx.x; i < k; i += kMtThreads) {
    m.c[3 * i] = cs[3 * i];
    m.c[3 * i + 1] = cs[3 * i + 1];
    m.c[3 * i + 2] = cs[3 * i + 2];
    const double x = fx * (double)ct[3 * i], y = fy * (double)ct[3 * i + 1], z = (double)ct[3 * i + 2];
    for (int j = 0; j < 3; ++j)                  // e rot^T
      m.e[3 * i + j] = (x * (double)rot[3 * j] + y * (double)rot[3 * j + 1] + z * (double)rot[3 * j + 2]) * scale;
    m.s[i] = mt_conf(sc + 2 * i);
  }
}

__device__ __forceinline__ int mt_argmax(const float *v, int n) {   // first index on ties, as torch.argmax
  int best = 0;
  float top = v[0];
  for (int j = 1; j < n; ++j) {
    if (v[j] > top) {
      top = v[j];
      best = j;
    }
  }
  return best;
}

__device__ __forceinline__ double mt_lse(const float *v, int n) {
  double m = (double)v[0];
  for (int j = 1; j < n; ++j) m = fmax(m, (double)v[j]);
  double s = 0.0;
  for (int j = 0; j < n; ++j) s += exp((double)v[j] - m);
  return m + log(s);
}

// sum_c pT[c] (log pT[c] - log pS[c]) of two rows of logits (F.kl_div's pointwise term, xlogy(0, 0) = 0)
__device__ __forceinline__ double mt_kl_row(const float *ls, const float *lt, int n) {
  const double lse_s = mt_lse(ls, n), lse_t = mt_lse(lt, n);
  double kl = 0.0;
  for (int j = 0; j < n; ++j) {
    const double lpt = (double)lt[j] - lse_t, pt = exp(lpt);
    if (pt > 0.0) kl += pt * (lpt - ((double)ls[j] - lse_s));
  }
  return kl;
}

// mean_size[cls] + size_residuals[row, cls] (:144-150)
__device__ __forceinline__ void mt_size(const float *mean_size, const float *residuals, size_t row, int ns, int cls, double scale,
                                        double *out) {
  for (int j = 0; j < 3; ++j)
    out[j] = ((double)mean_size[3 * cls + j] + (double)residuals[(row * ns + cls) * 3 + j]) * scale;
}

__device__ __forceinline__ int mt_cls(int cls, int ns) { return min(max(cls, 0), ns - 1); }

struct MtCos {
  double cos, xh0, xh1, yh0, yh1, nx;
};

// F.cosine_similarity of two 2-vectors: each divided by max(|.|, eps), then the dot product
__device__ __forceinline__ MtCos mt_cos(const float *x, const float *y) {
  MtCos r;
  const double x0 = (double)x[0], x1 = (double)x[1], y0 = (double)y[0], y1 = (double)y[1];
  r.nx = sqrt(x0 * x0 + x1 * x1);
  const double ny = sqrt(y0 * y0 + y1 * y1);
  const double dx = fmax(r.nx, kMtCosEps), dy = fmax(ny, kMtCosEps);
  r.xh0 = x0 / dx, r.xh1 = x1 / dx, r.yh0 = y0 / dy, r.yh1 = y1 / dy;
  r.cos = r.xh0 * r.yh0 + r.xh1 * r.yh1;
  return r;
}

__device__ __forceinline__ double mt_sq2(const float *a, const float *b) {
  const double d0 = (double)a[0] - (double)b[0], d1 = (double)a[1] - (double)b[1];
  return d0 * d0 + d1 * d1;
}

// sum over the workgroup in a fixed order: lanes by shuffles, then the waves' totals one after the other
__device__ __forceinline__ double mt_block_sum(double v, double *scratch) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();                                // scratch may still be read from the previous call
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kMtWaves; ++w) t += scratch[w];
  return t;
}

// grid (b, 2 prefixes)
__global__ __launch_bounds__(kMtThreads) void mt_rows_kernel(omnipq_mt_desc d, void *workspace, float *__restrict__ ema_center,
                                                            long long *__restrict__ assignment,
                                                            float *__restrict__ confidence) {
  extern __shared__ double s_dyn[];
  __shared__ double s_red[kMtWaves];
  const int b = (int)blockIdx.x, pk = (int)blockIdx.y, p = pk >> 1, quad = pk & 1, k = d.k, tid = (int)threadIdx.x;
  const MtScene m = mt_scene((unsigned char *)s_dyn, k);
  const MtWs w = mt_ws(workspace, d.prefixes, d.b, k);
  const size_t n = (size_t)d.b * k, row0 = (size_t)b * k, out0 = (size_t)pk * n + row0;
  mt_stage(d, b, p, quad, m);
  __syncthreads();
  for (int i = tid; i < k; i += kMtThreads) {
    for (int j = 0; j < 3; ++j) ema_center[(out0 + i) * 3 + j] = (float)m.e[3 * i + j];
    confidence[out0 + i] = (float)m.s[i];
  }
  // nn_distance (:44): items [0, k) the teacher centre nearest to student i, items [k, 2 k) the student nearest to teacher j
  for (int it = tid; it < 2 * k; it += kMtThreads) {
    const bool first = it < k;
    const int r = first ? it : it - k;
    double best = 0.0;
    int arg = 0;
    for (int o = 0; o < k; ++o) {
      const double dist = first ? mt_sq3(m.c + 3 * r, m.e + 3 * o) : mt_sq3(m.c + 3 * o, m.e + 3 * r);
      if (o == 0 || dist < best) {
        best = dist;
        arg = o;
      }
    }
    if (first) {
      m.d1[r] = best;
      m.i1[r] = arg;
    } else {
      m.d2[r] = best;
      m.i2[r] = arg;
    }
  }
  __syncthreads();
  float *v0 = w.vals + ((size_t)pk * 3 + 0) * n + row0, *v1 = w.vals + ((size_t)pk * 3 + 1) * n + row0,
        *v2 = w.vals + ((size_t)pk * 3 + 2) * n + row0;
  const double scale = (double)d.scale[b];
  double kl = 0.0;
  for (int r = tid; r < k; r += kMtThreads) {
    const int a = m.i2[r];
    const double conf = m.s[r];
    w.ind1[out0 + r] = m.i1[r];
    w.ind2[out0 + r] = a;
    assignment[out0 + r] = (long long)a;
    v0[r] = (float)(m.d1[r] * m.s[m.i1[r]] + m.d2[r] * conf);
    if (!quad) {
      const int ns = d.ns;
      const int cls_own = mt_argmax(d.size_scores[p] + (row0 + r) * ns, ns);
      const int cls_t = mt_argmax(d.t_size_scores[p] + (row0 + r) * ns, ns);
      const int cls_a = mt_argmax(d.size_scores[p] + (row0 + a) * ns, ns);
      w.cls[((size_t)p * 2 + 0) * n + row0 + r] = cls_own;
      w.cls[((size_t)p * 2 + 1) * n + row0 + r] = cls_t;
      double ss[3], st[3];
      mt_size(d.mean_size, d.size_residuals[p], row0 + a, ns, cls_a, 1.0, ss);
      mt_size(d.mean_size, d.t_size_residuals[p], row0 + r, ns, cls_t, scale, st);
      const double e0 = ss[0] - st[0], e1 = ss[1] - st[1], e2 = ss[2] - st[2];
      v1[r] = (float)((e0 * e0 + e1 * e1 + e2 * e2) * conf);
      v2[r] = 0.0f;
      kl += mt_kl_row(d.sem_cls_scores[p] + (row0 + a) * d.nc, d.t_sem_cls_scores[p] + (row0 + r) * d.nc, d.nc);
    } else {
      const MtCos cs = mt_cos(d.normal_vector[p] + (row0 + a) * 3, d.t_normal_vector[p] + (row0 + r) * 3);
      v1[r] = (float)((1.0 - fabs(cs.cos)) * conf);
      v2[r] = (float)(mt_sq2(d.quad_size[p] + (row0 + a) * 2, d.t_quad_size[p] + (row0 + r) * 2) * conf);
      kl += mt_kl_row(d.quad_scores[p] + (row0 + a) * 2, d.t_quad_scores[p] + (row0 + r) * 2, 2);
    }
  }
  kl = mt_block_sum(kl, s_red);
  if (tid == 0) w.kl[(size_t)pk * d.b + b] = kl;
}

// floats of either sign <-> keys that order like unsigned integers
__device__ __forceinline__ unsigned mt_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mt_unkey(float key) {
  const unsigned u = __float_as_uint(key);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// grid (2 prefixes): eps = quantile(values, 0.85), the masks [v < eps] and the masked sums of the arrays of one prefix and
// kind; the KL sum over the scenes in scene order
__global__ __launch_bounds__(kMtThreads) void mt_clip_kernel(int prefixes, int b, int k, void *workspace) {
  extern __shared__ float s_keys[];              // b * k
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_sel[4];
  __shared__ double s_red[kMtWaves];
  const int pk = (int)blockIdx.x, tid = (int)threadIdx.x, n = b * k;
  const MtWs w = mt_ws(workspace, prefixes, b, k);
  const int arrays = (pk & 1) ? 3 : 2;
  int below;
  float wt;
  quantile_rank(n, kMtClip, below, wt);
  for (int arr = 0; arr < 3; ++arr) {
    const float *vals = w.vals + ((size_t)pk * 3 + arr) * n;
    unsigned char *mask = w.mask + ((size_t)pk * 3 + arr) * n;
    if (arr >= arrays) {                          // uniform
      for (int i = tid; i < n; i += kMtThreads) mask[i] = 0;
      if (tid == 0) {
        w.rec[(size_t)pk * 4 + arr] = 0.0;
        w.eps[(size_t)pk * 4 + arr] = 0.0f;
      }
      continue;
    }
    __syncthreads();                              // the previous array's keys are no longer read
    for (int i = tid; i < n; i += kMtThreads) s_keys[i] = __uint_as_float(mt_key(vals[i]));
    __syncthreads();
    float lo, hi;
    radix_select<kMtThreads>(s_keys, n, below, s_hist, s_sel, lo, hi);
    const float eps = quantile_lerp(mt_unkey(lo), mt_unkey(hi), wt);
    double sum = 0.0;
    for (int i = tid; i < n; i += kMtThreads) {
      const float v = vals[i];
      const bool keep = v < eps;
      mask[i] = keep ? 1 : 0;
      if (keep) sum += (double)v;
    }
    sum = mt_block_sum(sum, s_red);
    if (tid == 0) {
      w.rec[(size_t)pk * 4 + arr] = sum;
      w.eps[(size_t)pk * 4 + arr] = eps;
    }
  }
  if (tid == 0) {
    double kl = 0.0;
    for (int s = 0; s < b; ++s) kl += w.kl[(size_t)pk * b + s];
    w.rec[(size_t)pk * 4 + 3] = kl;
    w.eps[(size_t)pk * 4 + 3] = 0.0f;
  }
}

// the terms of every prefix (:238, :249), summed in prefix order and divided by their number (:258-270)
__global__ __launch_bounds__(64) void mt_fold_kernel(int prefixes, int b, int k, int nc, const void *workspace,
                                                    float *__restrict__ terms) {
  if (threadIdx.x != 0) return;
  const MtWs w = mt_ws((void *)workspace, prefixes, b, k);
  const double n = (double)b * (double)k;
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < prefixes; ++p) {
    const double *o = w.rec + (size_t)(2 * p) * 4, *q = o + 4;
    const double centre = o[0] / n, cls = 2.0 * (o[3] / (n * nc)), size = o[1] / n;
    const double q_centre = q[0] / n, q_cls = 2.0 * (q[3] / b), q_normal = q[1] / n, q_size = q[2] / n;
    acc[0] += centre;
    acc[1] += cls;
    acc[2] += size;
    acc[3] += 0.5 * centre + 1.0 * cls + 0.05 * size;
    acc[4] += q_centre;
    acc[5] += q_cls;
    acc[6] += q_normal;
    acc[7] += q_size;
    acc[8] += 0.5 * q_centre + 0. * q_cls + 1.0 * q_normal + 0.05 * q_size;
  }
  for (int t = 0; t < 9; ++t) terms[t] = (float)(acc[t] / prefixes);
  terms[9] = (float)(acc[3] / prefixes + acc[8] / prefixes);
}

// grid (b, 2 prefixes).  The thread of student row i walks the scene's assignments in index order and gathers what lands on i.
__global__ __launch_bounds__(kMtThreads) void mt_grad_kernel(omnipq_mt_desc d, const void *workspace,
                                                            const float *__restrict__ g_terms, omnipq_mt_grads g) {
  extern __shared__ double s_dyn[];
  const int b = (int)blockIdx.x, pk = (int)blockIdx.y, p = pk >> 1, quad = pk & 1, k = d.k, tid = (int)threadIdx.x;
  const MtScene m = mt_scene((unsigned char *)s_dyn, k);
  // the teacher rows assigned to every student row, in index order: rows lst[start[i] .. start[i + 1]) land on row i
  int *start = (int *)((unsigned char *)s_dyn + (size_t)kMtSceneBytes * k), *lst = start + k + 1;
  unsigned char *m0 = (unsigned char *)(lst + k), *m1 = m0 + k, *m2 = m1 + k;
  const MtWs w = mt_ws((void *)workspace, d.prefixes, d.b, k);
  const size_t n = (size_t)d.b * k, row0 = (size_t)b * k, out0 = (size_t)pk * n + row0;
  mt_stage(d, b, p, quad, m);
  for (int i = tid; i < k; i += kMtThreads) {
    // the forward's assignments, clamped: a workspace that no forward filled must not send a read astray
    m.i1[i] = min(max(w.ind1[out0 + i], 0), k - 1);
    m.i2[i] = min(max(w.ind2[out0 + i], 0), k - 1);
    m0[i] = w.mask[((size_t)pk * 3 + 0) * n + row0 + i];
    m1[i] = w.mask[((size_t)pk * 3 + 1) * n + row0 + i];
    m2[i] = w.mask[((size_t)pk * 3 + 2) * n + row0 + i];
  }
  __syncthreads();
  for (int i = tid; i < k; i += kMtThreads) {
    m.d1[i] = mt_sq3(m.c + 3 * i, m.e + 3 * m.i1[i]);
    m.d2[i] = mt_sq3(m.c + 3 * m.i2[i], m.e + 3 * i);
    int landed = 0;
    for (int r = 0; r < k; ++r) landed += m.i2[r] == i ? 1 : 0;
    start[i + 1] = landed;
  }
  __syncthreads();
  if (tid == 0) {
    start[0] = 0;
    for (int i = 0; i < k; ++i) start[i + 1] += start[i];
  }
  __syncthreads();
  for (int i = tid; i < k; i += kMtThreads) {
    int pos = start[i];
    for (int r = 0; r < k; ++r)
      if (m.i2[r] == i) lst[pos++] = r;
  }
  __syncthreads();
  // dLoss / d(sum of each part of this prefix and kind), the term weights (:238, :249) and the means folded in
  const double inv_p = 1.0 / d.prefixes, nd = (double)d.b * (double)k;
  const double g_sum = quad ? (double)g_terms[8] + (double)g_terms[9] : (double)g_terms[3] + (double)g_terms[9];
  const int t0 = quad ? 4 : 0;
  const double w_centre = ((double)g_terms[t0] + 0.5 * g_sum) * inv_p / nd;
  const double w_cls = quad ? ((double)g_terms[5] + 0. * g_sum) * inv_p * 2.0 / d.b
                            : ((double)g_terms[1] + 1.0 * g_sum) * inv_p * 2.0 / (nd * d.nc);
  const double w_v1 = quad ? ((double)g_terms[6] + 1.0 * g_sum) * inv_p / nd : ((double)g_terms[2] + 0.05 * g_sum) * inv_p / nd;
  const double w_v2 = quad ? ((double)g_terms[7] + 0.05 * g_sum) * inv_p / nd : 0.0;
  const double scale = (double)d.scale[b];
  const int ns = d.ns, nc = quad ? 2 : d.nc;
  const float *logits_s = quad ? d.quad_scores[p] : d.sem_cls_scores[p];
  const float *logits_t = quad ? d.t_quad_scores[p] : d.t_sem_cls_scores[p];
  for (int i = tid; i < k; i += kMtThreads) {
    const size_t row = row0 + i;
    const double ci[3] = {(double)m.c[3 * i], (double)m.c[3 * i + 1], (double)m.c[3 * i + 2]};
    double gc[3] = {0.0, 0.0, 0.0}, gs = 0.0;
    if (m0[i]) {                                  // d[i] = dist1[i] s[ind1[i]] + dist2[i] s[i]
      const int j = m.i1[i];
      const double f = 2.0 * m.s[j];
      for (int x = 0; x < 3; ++x) gc[x] += f * (ci[x] - m.e[3 * j + x]);
      gs += m.d2[i];
    }
    double pt_sum[OMNIPQ_MT_MAX_CLASSES];
    for (int c = 0; c < nc; ++c) pt_sum[c] = 0.0;
    const int landed = start[i + 1] - start[i];
    double gv1[3] = {0.0, 0.0, 0.0}, gv2[2] = {0.0, 0.0};
    double own[3] = {0.0, 0.0, 0.0};
    int cls_i = 0;
    if (!quad) {
      cls_i = mt_cls(w.cls[((size_t)p * 2 + 0) * n + row], ns);
      mt_size(d.mean_size, d.size_residuals[p], row, ns, cls_i, 1.0, own);
    }
    for (int r = 0; r < k; ++r)
      if (m.i1[r] == i && m0[r]) gs += m.d1[r];
    // the costly part runs over the row's own list: lanes of a wave stay together instead of taking turns at their matches
    for (int q = start[i]; q < start[i + 1]; ++q) {
      const int r = lst[q];
      const size_t trow = row0 + r;
      if (m0[r]) {
        const double f = 2.0 * m.s[r];
        for (int x = 0; x < 3; ++x) gc[x] += f * (ci[x] - m.e[3 * r + x]);
      }
      const double lse_t = mt_lse(logits_t + trow * nc, nc);
      for (int c = 0; c < nc; ++c) pt_sum[c] += exp((double)logits_t[trow * nc + c] - lse_t);
      if (!quad) {
        if (m1[r]) {
          double st[3];
          mt_size(d.mean_size, d.t_size_residuals[p], trow, ns, mt_cls(w.cls[((size_t)p * 2 + 1) * n + trow], ns), scale, st);
          for (int x = 0; x < 3; ++x) gv1[x] += 2.0 * m.s[r] * (own[x] - st[x]);
        }
      } else {
        if (m1[r]) {
          const MtCos cs = mt_cos(d.normal_vector[p] + row * 3, d.t_normal_vector[p] + trow * 3);
          const double sg = cs.cos > 0.0 ? 1.0 : (cs.cos < 0.0 ? -1.0 : 0.0);
          double dc0, dc1;
          if (cs.nx > kMtCosEps) {
            dc0 = (cs.yh0 - cs.cos * cs.xh0) / cs.nx;
            dc1 = (cs.yh1 - cs.cos * cs.xh1) / cs.nx;
          } else {
            dc0 = cs.yh0 / kMtCosEps;
            dc1 = cs.yh1 / kMtCosEps;
          }
          gv1[0] += -sg * m.s[r] * dc0;
          gv1[1] += -sg * m.s[r] * dc1;
        }
        if (m2[r]) {
          const float *qs = d.quad_size[p] + row * 2, *qt = d.t_quad_size[p] + trow * 2;
          gv2[0] += 2.0 * m.s[r] * ((double)qs[0] - (double)qt[0]);
          gv2[1] += 2.0 * m.s[r] * ((double)qs[1] - (double)qt[1]);
        }
      }
    }
    gs *= w_centre;
    // the distances of teacher row i carry s[i] as a factor
    const size_t arow = row0 + m.i2[i];
    if (!quad) {
      if (m1[i]) {
        double ss[3], st[3];
        mt_size(d.mean_size, d.size_residuals[p], arow, ns, mt_cls(w.cls[((size_t)p * 2 + 0) * n + arow], ns), 1.0, ss);
        mt_size(d.mean_size, d.t_size_residuals[p], row, ns, mt_cls(w.cls[((size_t)p * 2 + 1) * n + row], ns), scale, st);
        const double e0 = ss[0] - st[0], e1 = ss[1] - st[1], e2 = ss[2] - st[2];
        gs += w_v1 * (e0 * e0 + e1 * e1 + e2 * e2);
      }
    } else {
      if (m1[i]) gs += w_v1 * (1.0 - fabs(mt_cos(d.normal_vector[p] + arow * 3, d.t_normal_vector[p] + row * 3).cos));
      if (m2[i]) gs += w_v2 * mt_sq2(d.quad_size[p] + arow * 2, d.t_quad_size[p] + row * 2);
    }
    const double si = m.s[i], ds = gs * si * (1.0 - si);
    const double lse_s = mt_lse(logits_s + row * nc, nc);
    float *g_centre = (quad ? g.quad_center[p] : g.center[p]) + row * 3;
    for (int x = 0; x < 3; ++x) g_centre[x] = (float)(w_centre * gc[x]);
    if (!quad) {
      g.objectness_scores[p][row * 2] = (float)-ds;
      g.objectness_scores[p][row * 2 + 1] = (float)ds;
      for (int c = 0; c < nc; ++c)
        g.sem_cls_scores[p][row * nc + c] = (float)(w_cls * (landed * exp((double)logits_s[row * nc + c] - lse_s) - pt_sum[c]));
      float *g_res = g.size_residuals[p] + row * ns * 3;
      for (int c = 0; c < ns; ++c)
        for (int x = 0; x < 3; ++x) g_res[c * 3 + x] = c == cls_i ? (float)(w_v1 * gv1[x]) : 0.0f;
    } else {
      const double k0 = w_cls * (landed * exp((double)logits_s[row * 2] - lse_s) - pt_sum[0]);
      const double k1 = w_cls * (landed * exp((double)logits_s[row * 2 + 1] - lse_s) - pt_sum[1]);
      g.quad_scores[p][row * 2] = (float)(k0 - ds);
      g.quad_scores[p][row * 2 + 1] = (float)(k1 + ds);
      g.normal_vector[p][row * 3] = (float)(w_v1 * gv1[0]);
      g.normal_vector[p][row * 3 + 1] = (float)(w_v1 * gv1[1]);
      g.normal_vector[p][row * 3 + 2] = 0.0f;
      g.quad_size[p][row * 2] = (float)(w_v2 * gv2[0]);
      g.quad_size[p][row * 2 + 1] = (float)(w_v2 * gv2[1]);
    }
  }
}

int mt_check_sizes(int prefixes, int b, int k) {
  if (b < 0 || k < 1 || prefixes < 1 || prefixes > OMNIPQ_MT_MAX_PREFIXES) return OMNIPQ_EINVAL;
  if (k > OMNIPQ_MT_MAX_K || (long long)b * k > OMNIPQ_MT_MAX_ROWS || b > 65535) return OMNIPQ_ETOOLARGE;
  return OMNIPQ_OK;
}

int mt_check(const omnipq_mt_desc *d) {
  if (!d) return OMNIPQ_EINVAL;
  if (d->nc < 1 || d->nc > OMNIPQ_MT_MAX_CLASSES || d->ns < 1 || d->ns > OMNIPQ_MT_MAX_CLASSES) return OMNIPQ_EINVAL;
  if (const int rc = mt_check_sizes(d->prefixes, d->b, d->k)) return rc;
  if (d->b == 0) return OMNIPQ_OK;
  for (int p = 0; p < d->prefixes; ++p) {
    if (!d->center[p] || !d->objectness_scores[p] || !d->sem_cls_scores[p] || !d->size_scores[p] || !d->size_residuals[p] ||
        !d->quad_center[p] || !d->quad_scores[p] || !d->normal_vector[p] || !d->quad_size[p] || !d->t_center[p] ||
        !d->t_sem_cls_scores[p] || !d->t_size_scores[p] || !d->t_size_residuals[p] || !d->t_quad_center[p] ||
        !d->t_quad_scores[p] || !d->t_normal_vector[p] || !d->t_quad_size[p])
      return OMNIPQ_EINVAL;
  }
  if (!d->flip_x || !d->flip_y || !d->rot_mat || !d->scale || !d->mean_size) return OMNIPQ_EINVAL;
  return OMNIPQ_OK;
}

}  // namespace
}  // namespace omnipq

extern "C" long long omnipq_mt_consistency_workspace_bytes(int prefixes, int b, int k) {
  if (omnipq::mt_check_sizes(prefixes, b, k)) return 0;
  return omnipq::mt_layout(prefixes, b, k).bytes;
}

extern "C" int omnipq_mt_consistency(const omnipq_mt_desc *d, float *ema_center, long long *assignment, float *confidence,
                                     void *workspace, float *terms, void *stream) {
  if (const int rc = omnipq::mt_check(d)) return rc;
  if (d->b == 0) return OMNIPQ_OK;
  if (!ema_center || !assignment || !confidence || !workspace || !terms) return OMNIPQ_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)d->b, (unsigned)(2 * d->prefixes));
  omnipq::mt_rows_kernel<<<grid, omnipq::kMtThreads, (size_t)omnipq::kMtSceneBytes * d->k, st>>>(*d, workspace, ema_center,
                                                                                                 assignment, confidence);
  OMNIPQ_LAUNCH_CHECK();
  omnipq::mt_clip_kernel<<<(unsigned)(2 * d->prefixes), omnipq::kMtThreads, (size_t)d->b * d->k * sizeof(float), st>>>(
      d->prefixes, d->b, d->k, workspace);
  OMNIPQ_LAUNCH_CHECK();
  omnipq::mt_fold_kernel<<<1, 64, 0, st>>>(d->prefixes, d->b, d->k, d->nc, workspace, terms);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_mt_consistency_grad(const omnipq_mt_desc *d, const void *workspace, const float *g_terms,
                                          const omnipq_mt_grads *g, void *stream) {
  if (const int rc = omnipq::mt_check(d)) return rc;
  if (d->b == 0) return OMNIPQ_OK;
  if (!workspace || !g_terms || !g) return OMNIPQ_EINVAL;
  for (int p = 0; p < d->prefixes; ++p) {
    if (!g->center[p] || !g->objectness_scores[p] || !g->sem_cls_scores[p] || !g->size_residuals[p] || !g->quad_center[p] ||
        !g->quad_scores[p] || !g->normal_vector[p] || !g->quad_size[p])
      return OMNIPQ_EINVAL;
  }
  const dim3 grid((unsigned)d->b, (unsigned)(2 * d->prefixes));
  const size_t lds = ((size_t)omnipq::kMtSceneBytes + 8 + 3) * d->k + 4;   // scene, assignment lists, masks
  omnipq::mt_grad_kernel<<<grid, omnipq::kMtThreads, lds, (hipStream_t)stream>>>(*d, workspace, g_terms, *g);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
