// Windowed statistics of the step's reported scalars (include/omnipq_optim.h: omnipq_stats_accumulate; reference
// train.py:580-586, the stat_dict loop with its `.item()` per key): one thread per entry adds the scalar its record points at
// into an f64 slot of its own.  No thread touches another's slot and every slot sees its calls in stream order, so the sums
// are the sequential f64 sums of the reference's Python floats -- no atomics, no host read, capturable.
#include "common.h"
#include "omnipq_optim.h"

namespace omnipq {

struct StatEntry {
  const void *src;
  int kind;      // 0 = f32, 1 = f64
  int mode;      // 0 = sum, 1 = last value
};

constexpr int kStatThreads = 256;
constexpr int kStatMax = 4096;

// accum: the optimiser's { micro, apply } word (written by its finalise launch, which precedes this one on the stream) or null
__global__ __launch_bounds__(kStatThreads) void stats_accumulate_kernel(int n, const StatEntry *__restrict__ entries,
                                                                        double *__restrict__ sums, double *__restrict__ last,
                                                                        long long *__restrict__ window,
                                                                        const long long *__restrict__ accum) {
  const int i = (int)(blockIdx.x * kStatThreads + threadIdx.x);
  const bool apply = accum == nullptr || accum[1] != 0;
  if (apply && i < n) {
    const StatEntry e = entries[i];
    const double x = e.kind == 1 ? *(const double *)e.src : (double)*(const float *)e.src;
    last[i] = x;
    sums[i] = e.mode == 1 ? x : sums[i] + x;
  }
  if (i == 0) {
    if (apply) window[0] += 1;
    window[1] += 1;
  }
}

}  // namespace omnipq

using namespace omnipq;

extern "C" int omnipq_stats_accumulate(int n, const void *entries, double *sums, double *last, long long *window,
                                       const long long *accum, void *stream) {
  static_assert(sizeof(StatEntry) == 16, "the statistics entry is part of the C ABI");
  if (n < 1 || n > kStatMax) return OMNIPQ_EINVAL;
  if (!entries || !sums || !last || !window) return OMNIPQ_EINVAL;
  const int grid = (n + kStatThreads - 1) / kStatThreads;
  stats_accumulate_kernel<<<grid, kStatThreads, 0, (hipStream_t)stream>>>(n, (const StatEntry *)entries, sums, last, window,
                                                                           accum);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
