// The uniform hash grid of the point-set queries (ball_query.hip: omnipq_ball_query_grid; point_normals.hip: omnipq_knn):
//   1. bq_cell_kernel: bucket = hash(cell) & (H - 1) per point                      (H = 8192 buckets per scene)
//   2. omnipq_sa_build_csr: points grouped by bucket
//   3. bq_sorted_xyz_kernel: coordinates in bucket order (candidate loads become contiguous)
// A bucket holds every point of its cells AND of unrelated cells with the same hash: a consumer either tolerates the extra
// candidates (the ball test rejects them) or compares the candidate's own cell with the cell it is scanning (k-NN).
// The kernels are `static`: each translation unit that includes this header launches its own copy.
#pragma once
#include "common.h"

namespace omnipq {

constexpr int kBqBuckets = 8192;

__device__ __forceinline__ int bq_cell(float x, float inv_h) { return (int)floorf(x * inv_h); }
__device__ __forceinline__ int bq_bucket(int cx, int cy, int cz) {
  return (int)(((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u) ^ ((unsigned)cz * 83492791u)) & (kBqBuckets - 1);
}

static __global__ __launch_bounds__(256) void bq_cell_kernel(long long total, float inv_h, const float *__restrict__ xyz,
                                                            int *__restrict__ bucket) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  bucket[i] = bq_bucket(bq_cell(xyz[i * 3 + 0], inv_h), bq_cell(xyz[i * 3 + 1], inv_h), bq_cell(xyz[i * 3 + 2], inv_h));
}

static __global__ __launch_bounds__(256) void bq_sorted_xyz_kernel(long long total, int n, const float *__restrict__ xyz,
                                                                  const int *__restrict__ order, float *__restrict__ sorted) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long base = (i / n) * n;
  const long long src = base + order[i];
  sorted[i * 3 + 0] = xyz[src * 3 + 0];
  sorted[i * 3 + 1] = xyz[src * 3 + 1];
  sorted[i * 3 + 2] = xyz[src * 3 + 2];
}

}  // namespace omnipq

extern "C" int omnipq_sa_build_csr(int b, int n, int m, int s, const int *idx, int *offsets, int *order, int *scratch,
                                   const omnipq_row_plan *plan, void *stream);
