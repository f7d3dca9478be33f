// Fused gradient clipping + AdamW step (include/omnipq_optim.h; reference train.py:562-566 with the optimiser of
// train.py:364-374): squared-norm partials -> finalise -> update, three launches over a device table of ALL parameter
// tensors.  Every hyper-parameter, the step count and the bias corrections are read from device memory, so a captured
// launch follows a learning-rate schedule on replay.  HBM-bound: the norm pass reads 4 bytes per parameter, the update
// reads 16 and writes 12.
//
// Gradient accumulation (the reference's step_freq, train.py:493-494 and :562-576) is the same three launches with one more
// flat buffer: the norm pass adds the micro-batch's gradient into an f32 accumulator laid out like exp_avg (reads 8, writes 4
// bytes per parameter; 4 and 4 on the first micro-batch, which overwrites), the finalise launch counts micro-batches in a device
// word and marks the k-th call as the applying one, and the update reads the accumulator where it read the gradient.  The
// templates below are the ONE body behind both families of entry points.
//
// Mean-teacher weight averaging (reference train.py:435-439 and :576) rides on the same launches (kEma): the finalise launch
// forms alpha = min(1 - 1/(global_step + 1), decay) from a device word and advances it, the update launch holds the new p in
// registers and reads and writes the teacher's copy next to it (8 more bytes per parameter instead of a launch of 12), and a
// few more workgroups average the parameters that have no gradient.
//
// Dynamic loss scaling (torch.amp.GradScaler's two tensors and torch._amp_update_scale_) is one more scalar recurrence in the
// finalise launch (kScaled): thread 0 divides the norm and the update's coefficient by the scale it reads from device memory
// and, on an applying call, backs the scale off or grows it.  The two streaming launches do not know it exists.
//
// The learning-rate schedule (reference utils/lr_scheduler.py: get_scheduler; train.py:566) is the last scalar recurrence of the
// step (kSched): thread 0 forms the coefficient rows with lr_now[g] instead of the staged rate and, on an applying call,
// counts one scheduler step and re-evaluates lr_now for the next one.  omnipq_adamw_sched_finalize is the superset entry point.
#include <math.h>
#include <stddef.h>

#include "common.h"
#include "omnipq_optim.h"

namespace omnipq {

struct AdamRec {
  float *param;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  long long numel;
  int group;
  int reserved;
};

typedef float adam_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAdamThreads = 256;
constexpr int kAdamQuantum = 4 * kAdamThreads;        // elements one pass of 16-byte vectors covers: chunk sizes are multiples

__device__ __forceinline__ unsigned phase16(const void *p) { return (unsigned)(((uintptr_t)p >> 2) & 3u); }

// sum over the workgroup in a fixed order (lane tree inside each wave, then the four wave totals left to right); valid in
// thread 0
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double waves[kAdamThreads / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  if (lane_id() == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kAdamThreads / 64; ++w) s += waves[w];
  }
  return s;
}

__device__ __forceinline__ double sq_acc(double acc, float g, float gs) {
  const double x = (double)(gs * g);
  return __builtin_fma(x, x, acc);
}

// an f32x4 at any 4-byte-aligned address (the accumulator segment of a chunk whose gradient sits at another phase)
struct __attribute__((packed, aligned(4))) adam_f32x4_any {
  float e[4];
};

// Squared-norm partial of one chunk, in ONE fixed order: the head (up to 3 elements in front of the gradient's first 16-byte
// boundary, lanes of wave 0), the tail (lanes of wave 1), then 16-byte vectors, four per thread and pass.  kAccum: the value
// that is squared is the running sum a = first ? g : sum + g, which is stored back; `sum` is the chunk's accumulator
// segment.  It shares the PARAMETER's phase, not necessarily the gradient's: where the two differ, the same elements go to the
// same threads and the accumulator moves through 4-byte-aligned accesses.
template <bool kAccum>
__device__ __forceinline__ void adamw_sqnorm_chunk(const float *__restrict__ g, float *__restrict__ sum, bool first, int len,
                                                   float gs, double *__restrict__ partial) {
  const int tid = (int)threadIdx.x;
  double acc = 0.0;
  if (len > 0) {
    int head = (int)((4u - phase16(g)) & 3u);
    head = head < len ? head : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    {
      int i = -1;
      if (tid < head) i = tid;
      if (tid >= 64 && tid < 64 + (len - tail0)) i = tail0 + tid - 64;
      if (i >= 0) {
        float a = g[i];
        if (kAccum) {
          if (!first) a = sum[i] + a;
          sum[i] = a;
        }
        acc = sq_acc(acc, a, gs);
      }
    }
    const adam_f32x4 *gv = (const adam_f32x4 *)(g + head);
    const bool together = kAccum && phase16(sum) == phase16(g);
    for (int j0 = 0; j0 < nvec; j0 += 4 * kAdamThreads) {
      adam_f32x4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * kAdamThreads + tid;
        x[u] = j < nvec ? gv[j] : adam_f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (kAccum) {
        if (together) {
          adam_f32x4 *sv = (adam_f32x4 *)(sum + head);
          if (!first) {
            adam_f32x4 s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int j = j0 + u * kAdamThreads + tid;
              s[u] = j < nvec ? sv[j] : adam_f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = s[u] + x[u];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * kAdamThreads + tid;
            if (j < nvec) sv[j] = x[u];
          }
        } else {
          adam_f32x4_any *sv = (adam_f32x4_any *)(sum + head);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * kAdamThreads + tid;
            if (j < nvec) {
              adam_f32x4_any s;
              if (!first) {
                s = sv[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) x[u][e] = s.e[e] + x[u][e];
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) s.e[e] = x[u][e];
              sv[j] = s;
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = sq_acc(acc, x[u][0], gs);
        acc = sq_acc(acc, x[u][1], gs);
        acc = sq_acc(acc, x[u][2], gs);
        acc = sq_acc(acc, x[u][3], gs);
      }
    }
  }
  const double s = block_sum_f64(acc);
  if (tid == 0) *partial = s;
}

// accum (kAccum): int64[2] = { micro-batches already summed, apply mark of the last finalise }
template <bool kAccum>
__global__ __launch_bounds__(kAdamThreads) void adamw_grad_sqnorm_kernel(const AdamRec *__restrict__ recs,
                                                                        const int *__restrict__ chunks, int chunk,
                                                                        const double *__restrict__ hyper, int ngroups,
                                                                        const float *exp_avg_base, float *sum_base,
                                                                        const long long *__restrict__ accum,
                                                                        double *__restrict__ partials) {
  const int *ck = chunks + 2 * (size_t)blockIdx.x;
  const AdamRec r = recs[ck[0]];
  const float gs = (float)hyper[8 * (size_t)ngroups + 1];
  const long long base = (long long)ck[1] * chunk;
  const long long left = r.numel - base;
  const int len = left < (long long)chunk ? (int)left : chunk;
  float *sum = nullptr;
  bool first = true;
  if (kAccum) {
    sum = sum_base + (r.exp_avg - exp_avg_base) + base;
    first = accum[0] == 0;
  }
  adamw_sqnorm_chunk<kAccum>(r.grad + base, sum, first, len, gs, partials + blockIdx.x);
}

// The schedule's value for scheduler step e and base rate b: include/omnipq_optim.h states the formulas and their operation
// order (the library is built with -ffp-contract=off: every product and sum below rounds on its own, as in Python).
__device__ __forceinline__ double lr_schedule_value(const omnipq_lr_schedule *__restrict__ s, long long e, double b) {
  const long long w = s->warmup_iters;
  long long k = e;
  if (w > 0) {
    if (e <= w) return b / s->multiplier * ((s->multiplier - 1.) * (double)e / (double)w + 1.);
    k = e - w;
  }
  if (s->kind == 0) {
    const double pi = 3.141592653589793;           // math.pi
    return s->eta_min + (b - s->eta_min) * (1. + cos(pi * (double)k / (double)s->t_max)) / 2.;
  }
  int n = s->n_milestones;
  n = n < 0 ? 0 : (n > 8 ? 8 : n);                 // whatever the device struct holds, the tables are not left
  int j = 0;
  while (j < n && s->milestones[j] <= k) ++j;      // bisect_right
  return b * s->gamma_pow[j];
}

// an applying call's scheduler.step(): one more step counted, lr_now of the NEXT step (thread 0)
__device__ __forceinline__ void lr_schedule_advance(const omnipq_lr_schedule *__restrict__ s, const double *__restrict__ base_lr,
                                                    long long *__restrict__ state, double *__restrict__ lr_now, int ngroups) {
  const long long e = state[0] + 1;
  state[0] = e;
  for (int g = 0; g < ngroups; ++g) lr_now[g] = lr_schedule_value(s, e, base_lr[g]);
}

__global__ __launch_bounds__(64) void lr_schedule_eval_kernel(int ngroups, const omnipq_lr_schedule *__restrict__ s,
                                                              const double *__restrict__ base_lr,
                                                              const long long *__restrict__ state,
                                                              double *__restrict__ lr_now) {
  const long long e = state[0];
  for (int g = (int)threadIdx.x; g < ngroups; g += 64) lr_now[g] = lr_schedule_value(s, e, base_lr[g]);
}

// ema_state (kEma): int64[1] = the global_step the NEXT averaging uses; ema_coef: float[2] = { alpha, beta } for the update
// scaler (kScaled): the dynamic loss scale S and its growth tracker; scaler_cfg: double[4] = { growth_factor, backoff_factor,
// growth_interval, 0 }.  The gradients arrive as S * g: the norm and the update's coefficient are divided by the S read at
// entry, and an applying call ends with the recurrence of torch._amp_update_scale_.
// sched (kSched): the schedule, base_lr and lr_now: one double per group, sched_state: int64[1] = scheduler steps so far.
template <bool kAccum, bool kEma, bool kScaled, bool kSched = false>
__global__ __launch_bounds__(kAdamThreads) void adamw_finalize_kernel(int nchunks, const double *__restrict__ partials,
                                                                     const double *__restrict__ hyper, int ngroups,
                                                                     int accum_steps, long long *__restrict__ counters,
                                                                     long long *__restrict__ accum,
                                                                     long long *__restrict__ ema_state,
                                                                     const double *__restrict__ scaler_cfg,
                                                                     omnipq_loss_scaler *__restrict__ scaler,
                                                                     float *__restrict__ result, float *__restrict__ coef,
                                                                     float *__restrict__ ema_coef,
                                                                     const omnipq_lr_schedule *__restrict__ sched = nullptr,
                                                                     const double *__restrict__ base_lr = nullptr,
                                                                     long long *__restrict__ sched_state = nullptr,
                                                                     double *__restrict__ lr_now = nullptr) {
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < nchunks; i += kAdamThreads) acc += partials[i];
  const double sum = block_sum_f64(acc);
  if (threadIdx.x != 0) return;
  const double *last = hyper + 8 * (size_t)ngroups;
  const float max_norm = (float)last[0];
  float gs = (float)last[1];
  float total_norm = (float)sqrt(sum);
  float scale = 1.f;
  if (kScaled) {
    scale = scaler->scale;
    const double inv = 1.0 / (double)scale;
    total_norm = (float)(sqrt(sum) * inv);           // the norm of the unscaled gradients
    gs = (float)(last[1] * inv);
  }
  const bool finite = isfinite(total_norm);
  if (kAccum) {
    // a micro-batch that is not the k-th only counts: the norm of the running sum is reported, nothing else is touched
    const long long micro = accum[0];
    if (micro >= 0 && micro < (long long)accum_steps - 1) {
      result[0] = total_norm;
      accum[0] = micro + 1;
      accum[1] = 0;
      return;
    }
    accum[0] = 0;
    accum[1] = 1;
  }
  if (kEma) {
    // every applying call averages, a skipped one included (train.py:576 does not look at the norm): alpha in f64, then the
    // two roundings to f32 that the arguments of omnipq_ema_update go through
    const long long step = ema_state[0];
    const double a = fmin(1.0 - 1.0 / (double)(step + 1), last[2]);
    ema_coef[0] = (float)a;
    ema_coef[1] = (float)(1.0 - a);
    ema_state[0] = step + 1;
  }
  if (kScaled) {
    // torch._amp_update_scale_ (ATen/native/cuda/AmpKernels.cu): float * double in f64, one rounding to f32
    if (!finite) {
      scaler->scale = (float)((double)scale * scaler_cfg[1]);
      scaler->growth_tracker = 0;
    } else {
      const int successful = scaler->growth_tracker + 1;
      if (successful == (int)scaler_cfg[2]) {
        const float grown = (float)((double)scale * scaler_cfg[0]);
        if (isfinite(grown)) scaler->scale = grown;
        scaler->growth_tracker = 0;
      } else {
        scaler->growth_tracker = successful;
      }
    }
  }
  // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1, in the norm's f32
  float clip = 1.f;
  if (max_norm > 0.f && finite) clip = fminf(1.f, max_norm / (total_norm + 1e-6f));
  result[0] = total_norm;
  result[1] = clip;
  result[2] = finite ? 0.f : 1.f;
  result[3] = gs * clip;
  if (!finite) {
    counters[1] += 1;
    if (kSched) lr_schedule_advance(sched, base_lr, sched_state, lr_now, ngroups);      // train.py:566 does not look at the norm
    return;
  }
  const long long t = counters[0] + 1;
  counters[0] = t;
  for (int g = 0; g < ngroups; ++g) {
    const double *h = hyper + 8 * (size_t)g;
    const double lr = kSched ? lr_now[g] : h[0], beta1 = h[1], beta2 = h[2], eps = h[3], wd = h[4];
    const double bc1 = 1.0 - pow(beta1, (double)t);
    const double bc2 = 1.0 - pow(beta2, (double)t);
    float *c = coef + 8 * (size_t)g;
    c[0] = (float)(1.0 - lr * wd);
    c[1] = (float)beta1;
    c[2] = (float)(1.0 - beta1);
    c[3] = (float)beta2;
    c[4] = (float)(1.0 - beta2);
    c[5] = (float)(lr / bc1);
    c[6] = (float)(1.0 / sqrt(bc2));
    c[7] = (float)eps;
  }
  if (kSched) lr_schedule_advance(sched, base_lr, sched_state, lr_now, ngroups);
}

struct AdamCoef {
  float decay, beta1, omb1, beta2, omb2, step, rbc2s, eps, gc;
};

// one element of torch.optim.AdamW's update in f32 (fused multiply-adds written out: the library is built with
// -ffp-contract=off)
__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, const AdamCoef &c) {
  const float gp = c.gc * g;
  const float pd = p * c.decay;
  m = __builtin_fmaf(c.beta1, m, c.omb1 * gp);
  v = __builtin_fmaf(c.beta2, v, (c.omb2 * gp) * gp);
  const float denom = __builtin_fmaf(sqrtf(v), c.rbc2s, c.eps);
  p = __builtin_fmaf(-c.step, m / denom, pd);
}

// the teacher's record of a parameter that is not in the optimiser's table: the segment layout of omnipq_ema_update
struct EmaOnlyRec {
  float *ema;
  const float *param;
  long long numel;
};

// one element of the reference's update_ema_variables, rounded like ema_update_kernel (sa_stage.hip): t = e * alpha in f32,
// then one fused multiply-add
__device__ __forceinline__ float ema1(float e, float p, float alpha, float beta) {
  const float t = e * alpha;
  return __builtin_fmaf(beta, p, t);
}

// four floats at a 4-byte-aligned address: one 16-byte access where the caller knows the address to be 16-byte aligned
__device__ __forceinline__ adam_f32x4 load_f32x4(const float *q, bool aligned16) {
  if (aligned16) return *(const adam_f32x4 *)q;
  const adam_f32x4_any a = *(const adam_f32x4_any *)q;
  return adam_f32x4{a.e[0], a.e[1], a.e[2], a.e[3]};
}

__device__ __forceinline__ void store_f32x4(float *q, adam_f32x4 x, bool aligned16) {
  if (aligned16) {
    *(adam_f32x4 *)q = x;
    return;
  }
  adam_f32x4_any a;
#pragma unroll
  for (int k = 0; k < 4; ++k) a.e[k] = x[k];
  *(adam_f32x4_any *)q = a;
}

// the averaging alone over one chunk, p as it is in memory: one coalesced dword per lane
__device__ __forceinline__ void ema_chunk(float *__restrict__ e, const float *__restrict__ p, int len, float alpha,
                                          float beta) {
  for (int i = (int)threadIdx.x; i < len; i += kAdamThreads) e[i] = ema1(e[i], p[i], alpha, beta);
}

// The 16-byte vectors of one chunk: p, g, m and v start on a 16-byte boundary, four vectors of each per thread and trip.
// kEma: the teacher's vector of a pass is loaded behind that pass's stores of p, m and v, into the registers its gradient has
// left -- held next to P, G, M and V from the start, the sixteen registers of E would cost a wave per SIMD.  kAligned: e
// shares that boundary; otherwise it moves through 4-byte-aligned accesses.
template <bool kEma, bool kAligned>
__device__ __forceinline__ void adam_vectors(float *p, const float *g, float *m, float *v, float *e, int nvec,
                                             const AdamCoef &c, float alpha, float beta) {
  const int tid = (int)threadIdx.x;
  adam_f32x4 *pv = (adam_f32x4 *)p;
  const adam_f32x4 *gv = (const adam_f32x4 *)g;
  adam_f32x4 *mv = (adam_f32x4 *)m;
  adam_f32x4 *vv4 = (adam_f32x4 *)v;
  for (int j0 = 0; j0 < nvec; j0 += 4 * kAdamThreads) {
    adam_f32x4 P[4], G[4], M[4], V[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * kAdamThreads + tid;
      if (j < nvec) {
        P[u] = pv[j];
        G[u] = gv[j];
        M[u] = mv[j];
        V[u] = vv4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * kAdamThreads + tid;
      if (j < nvec) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float pe = P[u][k], me = M[u][k], ve = V[u][k];
          adam1(pe, G[u][k], me, ve, c);
          P[u][k] = pe;
          M[u][k] = me;
          V[u][k] = ve;
        }
        pv[j] = P[u];
        mv[j] = M[u];
        vv4[j] = V[u];
        if (kEma) {
          adam_f32x4 E = load_f32x4(e + 4 * (size_t)j, kAligned);
#pragma unroll
          for (int k = 0; k < 4; ++k) E[k] = ema1(E[k], P[u][k], alpha, beta);
          store_f32x4(e + 4 * (size_t)j, E, kAligned);
        }
      }
    }
  }
}

// kAccum: the gradient is the chunk's segment of the accumulator (same offsets as exp_avg: always the vector path), and a
// call that finalise did not mark as the applying one changes nothing.
// kEma: workgroup c < nchunks also averages the teacher's copy ema_ptrs[record] of its chunk with the p it has just computed;
// workgroups from nchunks on average the chunks of `only` (parameters without a gradient).  A step skipped for a non-finite
// norm still averages, with p read from memory.  The teacher's chunk moves as 16-byte vectors where it shares p's phase and
// through 4-byte-aligned accesses where it does not; p, g, m and v keep their path either way.
template <bool kAccum, bool kEma>
__global__ __launch_bounds__(kAdamThreads) void adamw_update_kernel(const AdamRec *__restrict__ recs,
                                                                   float *const *__restrict__ ema_ptrs, int nchunks,
                                                                   const int *__restrict__ chunks, int chunk,
                                                                   const EmaOnlyRec *__restrict__ only,
                                                                   const int *__restrict__ only_chunks,
                                                                   const float *exp_avg_base, const float *sum_base,
                                                                   const long long *__restrict__ accum,
                                                                   const float *__restrict__ coef,
                                                                   const float *__restrict__ ema_coef,
                                                                   const float *__restrict__ result) {
  if (kAccum && accum[1] == 0) return;           // not the k-th micro-batch
  const bool skipped = result[2] != 0.f;         // non-finite gradient norm: the whole step is skipped
  if (!kEma && skipped) return;
  float alpha = 0.f, beta = 0.f;
  if (kEma) {
    alpha = ema_coef[0];
    beta = ema_coef[1];
    if ((int)blockIdx.x >= nchunks) {
      const int *ok = only_chunks + 2 * (size_t)((int)blockIdx.x - nchunks);
      const EmaOnlyRec o = only[ok[0]];
      const long long obase = (long long)ok[1] * chunk;
      const long long oleft = o.numel - obase;
      const int olen = oleft < (long long)chunk ? (int)oleft : chunk;
      if (olen > 0) ema_chunk(o.ema + obase, o.param + obase, olen, alpha, beta);
      return;
    }
  }
  const int *ck = chunks + 2 * (size_t)blockIdx.x;
  const AdamRec r = recs[ck[0]];
  const long long base = (long long)ck[1] * chunk;
  const long long left = r.numel - base;
  const int len = left < (long long)chunk ? (int)left : chunk;
  if (len <= 0) return;
  float *p = r.param + base;
  float *e = nullptr;
  if (kEma) {
    e = ema_ptrs[ck[0]] + base;
    if (skipped) {
      ema_chunk(e, p, len, alpha, beta);
      return;
    }
  }
  const float *cf = coef + 8 * (size_t)r.group;
  const AdamCoef c = {cf[0], cf[1], cf[2], cf[3], cf[4], cf[5], cf[6], cf[7], result[3]};
  const float *g = (kAccum ? sum_base + (r.exp_avg - exp_avg_base) : r.grad) + base;
  float *m = r.exp_avg + base;
  float *v = r.exp_avg_sq + base;
  const int tid = (int)threadIdx.x;
  const unsigned ph = phase16(p);
  if (phase16(g) != ph || phase16(m) != ph || phase16(v) != ph) {
    // the four tensors do not share a phase modulo 16 bytes: element by element (still one coalesced dword per lane)
    for (int i0 = 0; i0 < len; i0 += 4 * kAdamThreads) {
      float pp[4], gg[4], mm[4], vv[4], ee[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * kAdamThreads + tid;
        if (i < len) {
          pp[u] = p[i];
          gg[u] = g[i];
          mm[u] = m[i];
          vv[u] = v[i];
          if (kEma) ee[u] = e[i];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * kAdamThreads + tid;
        if (i < len) {
          adam1(pp[u], gg[u], mm[u], vv[u], c);
          p[i] = pp[u];
          m[i] = mm[u];
          v[i] = vv[u];
          if (kEma) e[i] = ema1(ee[u], pp[u], alpha, beta);
        }
      }
    }
    return;
  }
  int head = (int)((4u - ph) & 3u);
  head = head < len ? head : len;
  const int nvec = (len - head) >> 2;
  const int tail0 = head + 4 * nvec;
  {
    // the peeled head (lanes of wave 0) and tail (lanes of wave 1): at most three elements each
    int i = -1;
    if (tid < head) i = tid;
    if (tid >= 64 && tid < 64 + (len - tail0)) i = tail0 + tid - 64;
    if (i >= 0) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam1(pp, g[i], mm, vv, c);
      p[i] = pp;
      m[i] = mm;
      v[i] = vv;
      if (kEma) e[i] = ema1(e[i], pp, alpha, beta);
    }
  }
  // (the choice is uniform over the workgroup; it is made HERE, outside the loop: a branch on it inside the four passes made
  // the compiler carry copies of P, M and V across it -- 182 registers, two waves per SIMD)
  if (kEma && phase16(e) != ph)
    adam_vectors<kEma, false>(p + head, g + head, m + head, v + head, e + head, nvec, c, alpha, beta);
  else
    adam_vectors<kEma, true>(p + head, g + head, m + head, v + head, kEma ? e + head : nullptr, nvec, c, alpha, beta);
}

static bool bad_chunk(int chunk_elems) { return chunk_elems <= 0 || (chunk_elems % kAdamQuantum) != 0; }

}  // namespace omnipq

using namespace omnipq;

extern "C" int omnipq_adamw_check_table(int nrec, const void *records_host, int nchunks, const int *chunks_host,
                                        int ngroups, int chunk_elems) {
  static_assert(sizeof(AdamRec) == 48, "AdamRec layout is part of the C ABI");
  if (nrec < 0 || nchunks < 0 || ngroups < 1 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if ((nrec > 0 && !records_host) || (nchunks > 0 && !chunks_host)) return OMNIPQ_EINVAL;
  const AdamRec *recs = (const AdamRec *)records_host;
  for (int i = 0; i < nrec; ++i) {
    const AdamRec &r = recs[i];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq || r.numel < 0) return OMNIPQ_EINVAL;
    if (r.group < 0 || r.group >= ngroups) return OMNIPQ_EINVAL;
    if ((((uintptr_t)r.param | (uintptr_t)r.grad | (uintptr_t)r.exp_avg | (uintptr_t)r.exp_avg_sq) & 3u) != 0) return OMNIPQ_EINVAL;
  }
  for (int i = 0; i < nchunks; ++i) {
    const int rec = chunks_host[2 * (size_t)i], c = chunks_host[2 * (size_t)i + 1];
    if (rec < 0 || rec >= nrec || c < 0) return OMNIPQ_EINVAL;
    if ((long long)c * chunk_elems >= recs[rec].numel) return OMNIPQ_EINVAL;
  }
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_grad_sqnorm(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                                        const double *hyper, int ngroups, double *partials, void *stream) {
  if (nrec < 0 || nchunks < 0 || ngroups < 1 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if (!hyper) return OMNIPQ_EINVAL;
  if (nrec == 0 || nchunks == 0) return OMNIPQ_OK;
  if (!records || !chunks || !partials) return OMNIPQ_EINVAL;
  adamw_grad_sqnorm_kernel<false><<<nchunks, kAdamThreads, 0, (hipStream_t)stream>>>(
      (const AdamRec *)records, chunks, chunk_elems, hyper, ngroups, nullptr, nullptr, nullptr, partials);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_finalize(int nchunks, const double *partials, const double *hyper, int ngroups,
                                     long long *counters, float *result, float *coef, void *stream) {
  if (nchunks < 0 || ngroups < 1) return OMNIPQ_EINVAL;
  if (!hyper || !counters || !result || !coef || (nchunks > 0 && !partials)) return OMNIPQ_EINVAL;
  adamw_finalize_kernel<false, false, false><<<1, kAdamThreads, 0, (hipStream_t)stream>>>(
      nchunks, partials, hyper, ngroups, 1, counters, nullptr, nullptr, nullptr, nullptr, result, coef, nullptr);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_update(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                                   const float *coef, const float *result, void *stream) {
  if (nrec < 0 || nchunks < 0 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if (!coef || !result) return OMNIPQ_EINVAL;
  if (nrec == 0 || nchunks == 0) return OMNIPQ_OK;
  if (!records || !chunks) return OMNIPQ_EINVAL;
  adamw_update_kernel<false, false><<<nchunks, kAdamThreads, 0, (hipStream_t)stream>>>(
      (const AdamRec *)records, nullptr, nchunks, chunks, chunk_elems, nullptr, nullptr, nullptr, nullptr, nullptr, coef, nullptr,
      result);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

// ---- gradient accumulation: the same three launches on every micro-batch ----------------------------------------------------

extern "C" int omnipq_adamw_accum_sqnorm(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                                         const double *hyper, int ngroups, const float *exp_avg_base, float *acc_base,
                                         const long long *accum, double *partials, void *stream) {
  if (nrec < 0 || nchunks < 0 || ngroups < 1 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if (!hyper || !exp_avg_base || !acc_base || !accum) return OMNIPQ_EINVAL;
  if (nrec == 0 || nchunks == 0) return OMNIPQ_OK;
  if (!records || !chunks || !partials) return OMNIPQ_EINVAL;
  adamw_grad_sqnorm_kernel<true><<<nchunks, kAdamThreads, 0, (hipStream_t)stream>>>(
      (const AdamRec *)records, chunks, chunk_elems, hyper, ngroups, exp_avg_base, acc_base, accum, partials);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_accum_finalize(int nchunks, const double *partials, const double *hyper, int ngroups,
                                           int accum_steps, long long *counters, long long *accum, float *result, float *coef,
                                           void *stream) {
  if (nchunks < 0 || ngroups < 1 || accum_steps < 1) return OMNIPQ_EINVAL;
  if (!hyper || !counters || !accum || !result || !coef || (nchunks > 0 && !partials)) return OMNIPQ_EINVAL;
  adamw_finalize_kernel<true, false, false><<<1, kAdamThreads, 0, (hipStream_t)stream>>>(
      nchunks, partials, hyper, ngroups, accum_steps, counters, accum, nullptr, nullptr, nullptr, result, coef, nullptr);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_accum_update(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                                         const float *exp_avg_base, const float *acc_base, const long long *accum,
                                         const float *coef, const float *result, void *stream) {
  if (nrec < 0 || nchunks < 0 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if (!exp_avg_base || !acc_base || !accum || !coef || !result) return OMNIPQ_EINVAL;
  if (nrec == 0 || nchunks == 0) return OMNIPQ_OK;
  if (!records || !chunks) return OMNIPQ_EINVAL;
  adamw_update_kernel<true, false><<<nchunks, kAdamThreads, 0, (hipStream_t)stream>>>(
      (const AdamRec *)records, nullptr, nchunks, chunks, chunk_elems, nullptr, nullptr, exp_avg_base, acc_base, accum, coef,
      nullptr, result);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

// ---- mean-teacher weight averaging inside the finalise and update launches ------------------------------------------------

extern "C" int omnipq_adamw_check_ema_table(int nrec, const void *ema_ptrs_host, int n_only, const void *ema_only_host,
                                            int n_only_chunks, const int *only_chunks_host, int chunk_elems) {
  static_assert(sizeof(EmaOnlyRec) == 24, "the ema_only record is the segment layout of omnipq_ema_update");
  if (nrec < 0 || n_only < 0 || n_only_chunks < 0 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if ((nrec > 0 && !ema_ptrs_host) || (n_only > 0 && !ema_only_host) || (n_only_chunks > 0 && !only_chunks_host))
    return OMNIPQ_EINVAL;
  const uintptr_t *ptrs = (const uintptr_t *)ema_ptrs_host;
  for (int i = 0; i < nrec; ++i)
    if (!ptrs[i] || (ptrs[i] & 3u) != 0) return OMNIPQ_EINVAL;
  const EmaOnlyRec *only = (const EmaOnlyRec *)ema_only_host;
  for (int i = 0; i < n_only; ++i) {
    const EmaOnlyRec &o = only[i];
    if (!o.ema || !o.param || o.numel < 0) return OMNIPQ_EINVAL;
    if ((((uintptr_t)o.ema | (uintptr_t)o.param) & 3u) != 0) return OMNIPQ_EINVAL;
  }
  for (int i = 0; i < n_only_chunks; ++i) {
    const int rec = only_chunks_host[2 * (size_t)i], c = only_chunks_host[2 * (size_t)i + 1];
    if (rec < 0 || rec >= n_only || c < 0) return OMNIPQ_EINVAL;
    if ((long long)c * chunk_elems >= only[rec].numel) return OMNIPQ_EINVAL;
  }
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_ema_finalize(int nchunks, const double *partials, const double *hyper, int ngroups,
                                         int accum_steps, long long *counters, long long *accum, long long *ema_state,
                                         float *result, float *coef, float *ema_coef, void *stream) {
  if (nchunks < 0 || ngroups < 1 || accum_steps < 1) return OMNIPQ_EINVAL;
  if (!hyper || !counters || !ema_state || !result || !coef || !ema_coef || (nchunks > 0 && !partials)) return OMNIPQ_EINVAL;
  if (!accum && accum_steps != 1) return OMNIPQ_EINVAL;
  if (accum)
    adamw_finalize_kernel<true, true, false><<<1, kAdamThreads, 0, (hipStream_t)stream>>>(
        nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state, nullptr, nullptr, result, coef, ema_coef);
  else
    adamw_finalize_kernel<false, true, false><<<1, kAdamThreads, 0, (hipStream_t)stream>>>(
        nchunks, partials, hyper, ngroups, 1, counters, nullptr, ema_state, nullptr, nullptr, result, coef, ema_coef);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_adamw_ema_update(int nrec, int nchunks, const void *records, const void *ema_ptrs, const int *chunks,
                                       int chunk_elems, int n_only, int n_only_chunks, const void *ema_only,
                                       const int *only_chunks, const float *exp_avg_base, const float *acc_base,
                                       const long long *accum, const float *coef, const float *ema_coef, const float *result,
                                       void *stream) {
  if (nrec < 0 || nchunks < 0 || n_only < 0 || n_only_chunks < 0 || bad_chunk(chunk_elems)) return OMNIPQ_EINVAL;
  if (!coef || !ema_coef || !result) return OMNIPQ_EINVAL;
  if (accum && (!exp_avg_base || !acc_base)) return OMNIPQ_EINVAL;
  if ((nrec > 0 && (!records || !ema_ptrs)) || (nchunks > 0 && (!chunks || nrec == 0))) return OMNIPQ_EINVAL;
  if ((n_only > 0 && !ema_only) || (n_only_chunks > 0 && (!only_chunks || n_only == 0))) return OMNIPQ_EINVAL;
  if ((long long)nchunks + n_only_chunks > 0x7fffffffLL) return OMNIPQ_EINVAL;
  const int grid = nchunks + n_only_chunks;
  if (grid == 0) return OMNIPQ_OK;
  if (accum)
    adamw_update_kernel<true, true><<<grid, kAdamThreads, 0, (hipStream_t)stream>>>(
        (const AdamRec *)records, (float *const *)ema_ptrs, nchunks, chunks, chunk_elems, (const EmaOnlyRec *)ema_only,
        only_chunks, exp_avg_base, acc_base, accum, coef, ema_coef, result);
  else
    adamw_update_kernel<false, true><<<grid, kAdamThreads, 0, (hipStream_t)stream>>>(
        (const AdamRec *)records, (float *const *)ema_ptrs, nchunks, chunks, chunk_elems, (const EmaOnlyRec *)ema_only,
        only_chunks, nullptr, nullptr, nullptr, coef, ema_coef, result);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

// ---- dynamic loss scaling: the superset finalise ----------------------------------------------------------------------------

// the layout a binding builds the device struct from (the line format of omnipq_abi_records), held to the compiler's
extern "C" const char *omnipq_loss_scaler_record(void) {
  static_assert(sizeof(omnipq_loss_scaler) == 8 && sizeof(float) == 4 && sizeof(int) == 4, "omnipq_loss_scaler: size");
  static_assert(offsetof(omnipq_loss_scaler, scale) == 0, "omnipq_loss_scaler.scale: offset");
  static_assert(offsetof(omnipq_loss_scaler, growth_tracker) == 4, "omnipq_loss_scaler.growth_tracker: offset");
  return "struct omnipq_loss_scaler scale:f growth_tracker:i";
}

template <bool kAccum, bool kEma>
static void launch_scaled_finalize(int nchunks, const double *partials, const double *hyper, int ngroups, int accum_steps,
                                   long long *counters, long long *accum, long long *ema_state, float *ema_coef,
                                   const double *scaler_cfg, omnipq_loss_scaler *scaler_state, float *result, float *coef,
                                   hipStream_t stream) {
  adamw_finalize_kernel<kAccum, kEma, true><<<1, kAdamThreads, 0, stream>>>(
      nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state, scaler_cfg, scaler_state, result, coef,
      ema_coef);
}

extern "C" int omnipq_adamw_scaled_finalize(int nchunks, const double *partials, const double *hyper, int ngroups,
                                            int accum_steps, long long *counters, long long *accum, long long *ema_state,
                                            float *ema_coef, const double *scaler_cfg, omnipq_loss_scaler *scaler_state,
                                            float *result, float *coef, void *stream) {
  if (nchunks < 0 || ngroups < 1 || accum_steps < 1) return OMNIPQ_EINVAL;
  if (!hyper || !counters || !result || !coef || (nchunks > 0 && !partials)) return OMNIPQ_EINVAL;
  if (!scaler_cfg || !scaler_state) return OMNIPQ_EINVAL;
  if ((ema_state == nullptr) != (ema_coef == nullptr)) return OMNIPQ_EINVAL;
  if (!accum && accum_steps != 1) return OMNIPQ_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (accum && ema_state)
    launch_scaled_finalize<true, true>(nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state, ema_coef,
                                       scaler_cfg, scaler_state, result, coef, st);
  else if (accum)
    launch_scaled_finalize<true, false>(nchunks, partials, hyper, ngroups, accum_steps, counters, accum, nullptr, nullptr,
                                        scaler_cfg, scaler_state, result, coef, st);
  else if (ema_state)
    launch_scaled_finalize<false, true>(nchunks, partials, hyper, ngroups, 1, counters, nullptr, ema_state, ema_coef,
                                        scaler_cfg, scaler_state, result, coef, st);
  else
    launch_scaled_finalize<false, false>(nchunks, partials, hyper, ngroups, 1, counters, nullptr, nullptr, nullptr,
                                         scaler_cfg, scaler_state, result, coef, st);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

// ---- the learning-rate schedule: its record, its evaluation and the superset finalise -----------------------------------------

// the record line and the static_asserts that hold it to the compiler's layout: written by omni-pq_amd/build.py from the header
#include "plain_struct_records.inc"

extern "C" const char *omnipq_lr_schedule_record(void) { return omnipq_lr_schedule_record_text; }

extern "C" int omnipq_lr_schedule_max_milestones(void) {
  static_assert(sizeof(((omnipq_lr_schedule *)0)->milestones) == 8 * sizeof(long long) &&
                    sizeof(((omnipq_lr_schedule *)0)->gamma_pow) == 9 * sizeof(double),
                "omnipq_lr_schedule: one power of gamma more than milestones");
  return 8;
}

extern "C" int omnipq_lr_schedule_eval(int ngroups, const omnipq_lr_schedule *sched, const double *base_lr,
                                       const long long *sched_state, double *lr_now, void *stream) {
  if (ngroups < 1 || !sched || !base_lr || !sched_state || !lr_now) return OMNIPQ_EINVAL;
  lr_schedule_eval_kernel<<<1, 64, 0, (hipStream_t)stream>>>(ngroups, sched, base_lr, sched_state, lr_now);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

namespace {
struct FinalizeArgs {
  int nchunks;
  const double *partials, *hyper;
  int ngroups, accum_steps;
  long long *counters, *accum, *ema_state;
  float *ema_coef;
  const double *scaler_cfg;
  omnipq_loss_scaler *scaler_state;
  const omnipq_lr_schedule *sched;
  const double *base_lr;
  long long *sched_state;
  double *lr_now;
  float *result, *coef;
  hipStream_t stream;
};

// one template parameter per optional part, peeled off one at a time
template <bool... kDone>
static void launch_finalize(const FinalizeArgs &a, const bool *want) {
  if constexpr (sizeof...(kDone) == 4) {
    adamw_finalize_kernel<kDone...><<<1, kAdamThreads, 0, a.stream>>>(
        a.nchunks, a.partials, a.hyper, a.ngroups, a.accum_steps, a.counters, a.accum, a.ema_state, a.scaler_cfg, a.scaler_state,
        a.result, a.coef, a.ema_coef, a.sched, a.base_lr, a.sched_state, a.lr_now);
  } else {
    if (want[0])
      launch_finalize<kDone..., true>(a, want + 1);
    else
      launch_finalize<kDone..., false>(a, want + 1);
  }
}
}  // namespace

extern "C" int omnipq_adamw_sched_finalize(int nchunks, const double *partials, const double *hyper, int ngroups,
                                           int accum_steps, long long *counters, long long *accum, long long *ema_state,
                                           float *ema_coef, const double *scaler_cfg, omnipq_loss_scaler *scaler_state,
                                           const omnipq_lr_schedule *sched, const double *base_lr, long long *sched_state,
                                           double *lr_now, float *result, float *coef, void *stream) {
  if (nchunks < 0 || ngroups < 1 || accum_steps < 1) return OMNIPQ_EINVAL;
  if (!hyper || !counters || !result || !coef || (nchunks > 0 && !partials)) return OMNIPQ_EINVAL;
  if ((scaler_cfg == nullptr) != (scaler_state == nullptr)) return OMNIPQ_EINVAL;
  if ((ema_state == nullptr) != (ema_coef == nullptr)) return OMNIPQ_EINVAL;
  const int nsched = (sched != nullptr) + (base_lr != nullptr) + (sched_state != nullptr) + (lr_now != nullptr);
  if (nsched != 0 && nsched != 4) return OMNIPQ_EINVAL;
  if (!accum && accum_steps != 1) return OMNIPQ_EINVAL;
  const FinalizeArgs a = {nchunks, partials, hyper, ngroups, accum ? accum_steps : 1, counters, accum, ema_state, ema_coef,
                          scaler_cfg, scaler_state, sched, base_lr, sched_state, lr_now, result, coef, (hipStream_t)stream};
  const bool want[4] = {accum != nullptr, ema_state != nullptr, scaler_state != nullptr, sched != nullptr};
  launch_finalize<>(a, want);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
