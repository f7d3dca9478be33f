// Order statistics and torch.quantile's linear interpolation over an array in LDS, one workgroup of THREADS threads:
// shared by the gamma-mixture guide (gamma_guide.hip) and the mean-teacher consistency loss (consistency.hip).
#pragma once
#include "common.h"

namespace omnipq {

// Order statistics `rank` and `rank + 1` (0-based, ascending) of vals[0, cnt): non-negative floats, whose bit patterns
// order like unsigned integers (+inf marks a dropped sample and sorts last).  Radix selection, 8 bits per pass: a 256-bin
// histogram of the values that match the prefix found so far, then the bin that holds the rank.  Integer atomics only.
// hist: 256 words, sel: 4 words of LDS.  rank + 1 >= cnt: hi = lo.
template <int THREADS>
__device__ void radix_select(const float *vals, int cnt, int rank, unsigned *hist, unsigned *sel, float &lo, float &hi) {
  const int tid = (int)threadIdx.x;
  unsigned prefix = 0, mask = 0, r = (unsigned)rank;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < cnt; i += THREADS) {
      const unsigned key = __float_as_uint(vals[i]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {                               // lane l owns bins 4 l .. 4 l + 3
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned own = c0 + c1 + c2 + c3;
      unsigned incl = own;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        if (tid >= d) incl += up;
      }
      unsigned below = incl - own;
      const unsigned c[4] = {c0, c1, c2, c3};
      for (int j = 0; j < 4; ++j) {
        if (r >= below && r < below + c[j]) {
          sel[0] = (unsigned)(4 * tid + j);
          sel[1] = r - below;
        }
        below += c[j];
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 255u << shift;
    r = sel[1];
  }
  // the next order statistic: the same value if it occurs beyond the rank, else the smallest larger one
  if (tid == 0) {
    sel[2] = 0;
    sel[3] = 0xffffffffu;
  }
  __syncthreads();
  unsigned le = 0, next = 0xffffffffu;
  for (int i = tid; i < cnt; i += THREADS) {
    const unsigned key = __float_as_uint(vals[i]);
    if (key <= prefix) ++le;
    else next = min(next, key);
  }
  atomicAdd(&sel[2], le);
  atomicMin(&sel[3], next);
  __syncthreads();
  lo = __uint_as_float(prefix);
  hi = (rank + 1 >= cnt || (unsigned)(rank + 1) < sel[2]) ? lo : __uint_as_float(sel[3]);
  __syncthreads();                                // sel is free again
}

// torch.quantile's rank of t among n values, in f32: the order statistic below it and the interpolation weight
__device__ __forceinline__ void quantile_rank(int n, float t, int &below, float &w) {
  const float rank = t * (float)(n - 1);
  const float fl = floorf(rank);
  below = (int)fl;
  w = rank - fl;
}

// Tensor.lerp's formula between the two bracketing order statistics
__device__ __forceinline__ float quantile_lerp(float lo, float hi, float w) {
  if (!(w > 0.0f)) return lo;
  const float diff = hi - lo;
  return w < 0.5f ? lo + w * diff : hi - diff * (1.0f - w);
}

// torch.quantile(vals, t) with the default linear interpolation: rank = t (n_k - 1) in f32, Tensor.lerp's formula
template <int THREADS>
__device__ float radix_quantile(const float *vals, int cnt, int n_k, float t, unsigned *hist, unsigned *sel) {
  int below;
  float w;
  quantile_rank(n_k, t, below, w);
  float lo, hi;
  radix_select<THREADS>(vals, cnt, below, hist, sel, lo, hi);
  return quantile_lerp(lo, hi, w);
}

}  // namespace omnipq
