// Per-point normals for gfx950: k nearest neighbours, plane fit, smoothing, orientation (include/omnipq_normals.h states the
// contract of the four stages; it replaces the offline MeshLab step of scannet/compute_normal_for_pc.py:29-48).
//
// knn is the hot path: at the recipe's size every one of 50 000 points wants its 100 nearest.  The points go into the hash
// grid of csrc/hash_grid.h (cell edge h, an argument).  One WAVE owns a query, four per workgroup, nothing crosses waves:
//   * shell s = 1, 2, 3: the (2 s + 1)^3 cells around the query's cell, 64 cells at a time (their bucket ranges laid end to
//     end by a prefix sum, as bq_grid_kernel does for its 27), 64 candidates at a time.  A candidate counts only in the cell
//     its OWN coordinates fall into, so cells that share a bucket and strangers in a bucket never show up twice.
//   * every point within the guaranteed radius r_g = (s - 0.01) h lies in those cells: fl(x / h) is off by < 2.5e-4 cells
//     while |x| / h < ~2000 (the `far` test), and the f32 d2 is within 1e-6 of the true one, both far inside the 0.01 margin.
//     So the candidates with d2 <= r_g^2 are ALL points with d2 <= r_g^2, and once there are k of them the k nearest are
//     among them.  Only those are kept (LDS, kKnnCap per wave).
//   * more of them than the list holds: the same selection with the candidates recomputed from the same cells on every
//     pass instead of read from LDS (nothing is written past the list's end).
//   * fewer than k after shell 3, or a far query: the exact walk -- the same selection over all n points, recomputed.
//   * selection: radix over the bit pattern of d2 (non-negative floats order as unsigned integers, csrc/radix_select.h),
//     8 bits a pass into a wave-private 256-bin histogram; everything below the k-th key wins, and of the ties at it the
//     lowest indices (a second radix selection over the index, only when there are more ties than places); the <= 128
//     winners are ranked by (d2, index) and stored in order.
// Every loop is bounded by n, k, the bucket ranges or a constant; no wave waits for another; every LDS slot is checked
// against its capacity and every gathered index against [0, n) before use.
#include "common.h"
#include "hash_grid.h"
#include "omnipq_normals.h"

namespace omnipq {

constexpr int kKnnMaxK = 128;
constexpr int kKnnCap = 1024;         // candidates kept per query before the walk
constexpr int kKnnShellMax = 3;       // S_MAX

struct KnnWave {
  unsigned key[kKnnCap];
  int idx[kKnnCap];
  unsigned hist[256];
  unsigned wkey[kKnnMaxK];
  int widx[kKnnMaxK];
  int cell_beg[64], cell_pre[64];
};

// LDS written by some lanes of a wave and read by others: the wave's DS operations execute in order, this keeps the
// compiler from moving them across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

enum { kFromList = 0, kFromGrid = 1, kFromWalk = 2 };

struct KnnQuery {
  int mode;                 // where the candidates come from: the cached list, the grid again, or all n points
  int total;                // list: cached candidates; walk: n
  int n;
  float qx, qy, qz;
  const float *xyz;         // walk
  int shell, cx, cy, cz;    // grid: the (2 shell + 1)^3 cells around (cx, cy, cz), candidates with d2 <= rg2
  float inv_h, rg2;
  const float *sorted;
  const int *offsets, *order;
};

// f(hit, key, index) for every point in the cells of q.shell, 64 at a time with all lanes active (f may ballot); hit: the
// point lies in the cell being scanned (not a stranger in its bucket) and within the guaranteed radius
template <typename F>
__device__ __forceinline__ void knn_grid_for_each(const KnnQuery &q, KnnWave &w, int lane, F f) {
  const int s = q.shell, side = 2 * s + 1, ncell = side * side * side;
  for (int g0 = 0; g0 < ncell; g0 += 64) {
    const int c = g0 + lane;
    const bool vc = c < ncell;
    const int bucket = vc ? bq_bucket(q.cx + c % side - s, q.cy + (c / side) % side - s, q.cz + c / (side * side) - s) : 0;
    const int beg = vc ? q.offsets[bucket] : 0;
    int num = vc ? q.offsets[bucket + 1] - beg : 0;
    if (num < 0 || beg < 0 || beg > q.n - num) num = 0;     // never trust a range beyond the scene
    int pre = num;                                        // inclusive prefix over the 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(pre, d, 64);
      if (lane >= d) pre += y;
    }
    const int total = __builtin_amdgcn_readlane(pre, 63);
    wave_sync();
    w.cell_beg[lane] = beg;
    w.cell_pre[lane] = pre - num;                         // exclusive
    wave_sync();
    for (int t0 = 0; t0 < total; t0 += 64) {
      const int t = t0 + lane;
      const bool valid = t < total;
      int ci = 0;                                         // the last cell whose exclusive prefix is <= t: the one that holds t
      if (valid) {
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
          if (ci + step < 64 && w.cell_pre[ci + step] <= t) ci += step;
      }
      const int pos = valid ? w.cell_beg[ci] + (t - w.cell_pre[ci]) : 0;
      const float x = q.sorted[(size_t)pos * 3 + 0], y = q.sorted[(size_t)pos * 3 + 1], z = q.sorted[(size_t)pos * 3 + 2];
      const int gc = g0 + ci;
      const bool own = bq_cell(x, q.inv_h) == q.cx + gc % side - s && bq_cell(y, q.inv_h) == q.cy + (gc / side) % side - s &&
                       bq_cell(z, q.inv_h) == q.cz + gc / (side * side) - s;
      const float d2 = sumsq3(q.qx - x, q.qy - y, q.qz - z);
      const bool hit = valid && own && d2 <= q.rg2;
      f(hit, __float_as_uint(d2), hit ? q.order[pos] : 0);
    }
  }
}

// f(valid, key, index) for every candidate, 64 at a time, with all lanes active (f may ballot)
template <typename F>
__device__ __forceinline__ void knn_for_each(const KnnQuery &q, KnnWave &w, int lane, F f) {
  if (q.mode == kFromGrid) {
    knn_grid_for_each(q, w, lane, f);
    return;
  }
  for (int i0 = 0; i0 < q.total; i0 += 64) {
    const int i = i0 + lane;
    const bool valid = i < q.total;
    unsigned key = 0;
    int id = 0;
    if (q.mode == kFromWalk) {
      const int ic = valid ? i : q.total - 1;
      key = __float_as_uint(sumsq3(q.qx - q.xyz[(size_t)ic * 3 + 0], q.qy - q.xyz[(size_t)ic * 3 + 1],
                                   q.qz - q.xyz[(size_t)ic * 3 + 2]));
      id = i;
    } else if (valid) {
      key = w.key[i];
      id = w.idx[i];
    }
    f(valid, key, id);
  }
}

// The value of 0-based rank `r` among the 32-bit values get(valid, key, index, v) admits.  On return r is the rank among the
// candidates that equal the result and `equal` their number.  The caller guarantees r < number admitted.
template <typename G>
__device__ __forceinline__ unsigned knn_radix_select(const KnnQuery &q, KnnWave &w, int lane, unsigned &r, unsigned &equal,
                                                     G get) {
  unsigned prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) w.hist[lane + 64 * j] = 0;
    wave_sync();
    knn_for_each(q, w, lane, [&](bool valid, unsigned key, int id) {
      unsigned v = 0;
      if (get(valid, key, id, v) && (v & mask) == prefix) atomicAdd(&w.hist[(v >> shift) & 255u], 1u);
    });
    wave_sync();
    const unsigned c[4] = {w.hist[4 * lane], w.hist[4 * lane + 1], w.hist[4 * lane + 2], w.hist[4 * lane + 3]};
    const unsigned own = c[0] + c[1] + c[2] + c[3];
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    unsigned below = incl - own;
    const bool mine = r >= below && r < below + own;
    unsigned bin = 0, rn = 0, cb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (mine && r >= below && r < below + c[j]) {
        bin = (unsigned)(4 * lane + j);
        rn = r - below;
        cb = c[j];
      }
      below += c[j];
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __builtin_ctzll(who) : 0;
    bin = __shfl(bin, src, 64);
    r = __shfl(rn, src, 64);
    equal = __shfl(cb, src, 64);
    prefix |= bin << shift;
    mask |= 255u << shift;
    wave_sync();                                          // the histogram is free again
  }
  return prefix;
}

__global__ __launch_bounds__(256) void knn_kernel(int n, int m, int k, float cell, float inv_h,
                                                 const float *__restrict__ new_xyz, const float *__restrict__ xyz,
                                                 const float *__restrict__ sorted, const int *__restrict__ offsets,
                                                 const int *__restrict__ order, int *__restrict__ idx,
                                                 float *__restrict__ dist2) {
  __shared__ KnnWave lds[4];
  const int scene = (int)blockIdx.y;
  const int wave = (int)(threadIdx.x >> 6);
  const int lane = lane_id();
  const long long qi = (long long)blockIdx.x * 4 + wave;
  if (qi >= m) return;                                  // whole wave; no workgroup barriers below
  KnnWave &w = lds[wave];
  xyz += (size_t)scene * n * 3;
  sorted += (size_t)scene * n * 3;
  order += (size_t)scene * n;
  offsets += (size_t)scene * (kBqBuckets + 1);
  new_xyz += ((size_t)scene * m + qi) * 3;
  idx += ((size_t)scene * m + qi) * k;
  if (dist2) dist2 += ((size_t)scene * m + qi) * k;
  KnnQuery q;
  q.n = n;
  q.xyz = xyz;
  q.sorted = sorted;
  q.offsets = offsets;
  q.order = order;
  q.inv_h = inv_h;
  q.qx = new_xyz[0];
  q.qy = new_xyz[1];
  q.qz = new_xyz[2];
  const unsigned long long lower = (1ull << lane) - 1ull;
  // the cell of a coordinate is exact to 2.5e-4 cells only while |x| / h < ~2000 (false for NaN too): beyond, the walk
  const bool far = !(fabsf(q.qx) * inv_h < 2000.f && fabsf(q.qy) * inv_h < 2000.f && fabsf(q.qz) * inv_h < 2000.f);

  int cnt = 0;
  bool done = false;
  if (!far) {
    q.cx = bq_cell(q.qx, inv_h), q.cy = bq_cell(q.qy, inv_h), q.cz = bq_cell(q.qz, inv_h);
    for (int s = 1; s <= kKnnShellMax && !done; ++s) {
      const float rg = cell * ((float)s - 0.01f);
      q.shell = s;
      q.rg2 = rg * rg;
      cnt = 0;
      knn_grid_for_each(q, w, lane, [&](bool hit, unsigned key, int id) {
        const unsigned long long hits = __ballot(hit);
        if (hits) {
          const int slot = cnt + __builtin_popcountll(hits & lower);
          if (hit && slot < kKnnCap) {                    // past the list's end: counted, not stored
            w.key[slot] = key;
            w.idx[slot] = id;
          }
          cnt += __builtin_popcountll(hits);
        }
      });
      done = cnt >= k;
    }
  }
  wave_sync();
  // k candidates within the guaranteed radius: from the list where they fit, from the grid again where they do not
  q.mode = !done ? kFromWalk : cnt > kKnnCap ? kFromGrid : kFromList;
  q.total = done ? cnt : n;
  const int kk = k < q.total ? k : q.total;
  if (kk > 0) {
    auto any_key = [](bool valid, unsigned key, int, unsigned &v) {
      v = key;
      return valid;
    };
    unsigned r = (unsigned)(kk - 1), ties = 0;
    const unsigned kth = knn_radix_select(q, w, lane, r, ties, any_key);
    unsigned last = 0xffffffffu;                          // every tie wins unless there are more than places
    if (ties > r + 1) {
      unsigned r2 = r, same = 0;
      last = knn_radix_select(q, w, lane, r2, same, [kth](bool valid, unsigned key, int id, unsigned &v) {
        v = (unsigned)id;
        return valid && key == kth;
      });
    }
    int found = 0;
    knn_for_each(q, w, lane, [&](bool valid, unsigned key, int id) {
      const bool win = valid && (key < kth || (key == kth && (unsigned)id <= last));
      const unsigned long long wins = __ballot(win);
      if (wins) {
        const int slot = found + __builtin_popcountll(wins & lower);
        if (win && slot < kKnnMaxK) {
          w.wkey[slot] = key;
          w.widx[slot] = id;
        }
        found += __builtin_popcountll(wins);
      }
    });
    wave_sync();
    const int have = found < kk ? found : kk;             // == kk: exactly kk candidates are <= (kth, last)
    for (int i = lane; i < have; i += 64) {
      const unsigned ki = w.wkey[i];
      const int ii = w.widx[i];
      int rank = 0;
      for (int j = 0; j < have; ++j) {
        const unsigned kj = w.wkey[j];
        rank += (kj < ki || (kj == ki && w.widx[j] < ii)) ? 1 : 0;
      }
      if (rank < k) {
        idx[rank] = ii;
        if (dist2) dist2[rank] = __uint_as_float(ki);
      }
    }
  }
  for (int s = kk + lane; s < k; s += 64) {               // fewer than k points: -1 / +inf
    idx[s] = -1;
    if (dist2) dist2[s] = __uint_as_float(0x7f800000u);
  }
}

__global__ __launch_bounds__(256) void knn_empty_kernel(long long total, int *__restrict__ idx, float *__restrict__ dist2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  idx[i] = -1;
  if (dist2) dist2[i] = __uint_as_float(0x7f800000u);
}

// ---- plane fit ---------------------------------------------------------------------------------------------------------
// one Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q); r is the third index.  A <- J^T A J, V <- V J:
// the classical formulas with t = tan of the rotation angle, the smaller root.
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                              double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  double vp = v0p, vq = v0q;
  v0p = c * vp - s * vq;
  v0q = s * vp + c * vq;
  vp = v1p, vq = v1q;
  v1p = c * vp - s * vq;
  v1q = s * vp + c * vq;
  vp = v2p, vq = v2q;
  v2p = c * vp - s * vq;
  v2q = s * vp + c * vq;
}

constexpr int kJacobiSweeps = 10;

__global__ __launch_bounds__(256) void plane_fit_kernel(long long total, int n, int k, const float *__restrict__ xyz,
                                                       const int *__restrict__ idx, float *__restrict__ normals,
                                                       double *__restrict__ eig) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float *pts = xyz + (i / n) * n * 3;
  const int *row = idx + i * k;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0;
  for (int j = 0; j < k; ++j) {
    const int e = row[j];
    if (e < 0 || e >= n) continue;
    sx += (double)pts[(size_t)e * 3 + 0];
    sy += (double)pts[(size_t)e * 3 + 1];
    sz += (double)pts[(size_t)e * 3 + 2];
    ++cnt;
  }
  double a00 = 0.0, a11 = 0.0, a22 = 0.0, a01 = 0.0, a02 = 0.0, a12 = 0.0;
  if (cnt > 0) {
    const double dc = (double)cnt;
    const double mx = sx / dc, my = sy / dc, mz = sz / dc;
    for (int j = 0; j < k; ++j) {
      const int e = row[j];
      if (e < 0 || e >= n) continue;
      const double dx = (double)pts[(size_t)e * 3 + 0] - mx;
      const double dy = (double)pts[(size_t)e * 3 + 1] - my;
      const double dz = (double)pts[(size_t)e * 3 + 2] - mz;
      a00 += dx * dx;
      a11 += dy * dy;
      a22 += dz * dz;
      a01 += dx * dy;
      a02 += dx * dz;
      a12 += dy * dz;
    }
    a00 /= dc, a11 /= dc, a22 /= dc, a01 /= dc, a02 /= dc, a12 /= dc;
  }
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0, 1), r = 2
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2), r = 1
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2), r = 0
  }
  // the column of the smallest eigenvalue, the first among equal ones
  double l0 = a00, ex = v00, ey = v10, ez = v20;
  if (a11 < l0) l0 = a11, ex = v01, ey = v11, ez = v21;
  if (a22 < l0) l0 = a22, ex = v02, ey = v12, ez = v22;
  float fx = (float)ex, fy = (float)ey, fz = (float)ez;
  float big = fx;
  if (fabsf(fy) > fabsf(big)) big = fy;
  if (fabsf(fz) > fabsf(big)) big = fz;
  if (big < 0.f) fx = -fx, fy = -fy, fz = -fz;
  normals[i * 3 + 0] = fx;
  normals[i * 3 + 1] = fy;
  normals[i * 3 + 2] = fz;
  if (eig) {
    double lo = a00, mid = a11, hi = a22, tmp;
    if (mid < lo) tmp = lo, lo = mid, mid = tmp;
    if (hi < mid) tmp = mid, mid = hi, hi = tmp;
    if (mid < lo) tmp = lo, lo = mid, mid = tmp;
    eig[i * 3 + 0] = lo;
    eig[i * 3 + 1] = mid;
    eig[i * 3 + 2] = hi;
  }
}

// ---- smoothing step and orientation ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smooth_kernel(long long total, int n, int k, const int *__restrict__ idx,
                                                    const float *__restrict__ in, float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float *nrm = in + (i / n) * n * 3;
  const int *row = idx + i * k;
  const float fx = in[i * 3 + 0], fy = in[i * 3 + 1], fz = in[i * 3 + 2];
  const double nx = (double)fx, ny = (double)fy, nz = (double)fz;
  double tx = 0.0, ty = 0.0, tz = 0.0;
  for (int j = 0; j < k; ++j) {
    const int e = row[j];
    if (e < 0 || e >= n) continue;
    const double ox = (double)nrm[(size_t)e * 3 + 0], oy = (double)nrm[(size_t)e * 3 + 1], oz = (double)nrm[(size_t)e * 3 + 2];
    const double dot = (nx * ox + ny * oy) + nz * oz;
    if (dot > 0.0) {
      tx += ox, ty += oy, tz += oz;
    } else {
      tx -= ox, ty -= oy, tz -= oz;
    }
  }
  float rx = fx, ry = fy, rz = fz;
  if (tx != 0.0 || ty != 0.0 || tz != 0.0) {
    const double len = sqrt((tx * tx + ty * ty) + tz * tz);
    rx = (float)(tx / len);
    ry = (float)(ty / len);
    rz = (float)(tz / len);
  }
  out[i * 3 + 0] = rx;
  out[i * 3 + 1] = ry;
  out[i * 3 + 2] = rz;
}

__global__ __launch_bounds__(256) void orient_kernel(long long total, int n, const float *__restrict__ xyz,
                                                    const double *__restrict__ centre, float *__restrict__ normals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double *c = centre + (i / n) * 3;
  const float fx = normals[i * 3 + 0], fy = normals[i * 3 + 1], fz = normals[i * 3 + 2];
  const double dot = (((double)xyz[i * 3 + 0] - c[0]) * (double)fx + ((double)xyz[i * 3 + 1] - c[1]) * (double)fy) +
                     ((double)xyz[i * 3 + 2] - c[2]) * (double)fz;
  if (dot < 0.0) {
    normals[i * 3 + 0] = -fx;
    normals[i * 3 + 1] = -fy;
    normals[i * 3 + 2] = -fz;
  }
}

static bool normals_sizes_ok(int b, int n, int k) { return b >= 0 && n >= 0 && k >= 1 && k <= kKnnMaxK && b <= 65535; }
static unsigned blocks_for(long long total) { return (unsigned)((total + 255) / 256); }
// one launch covers at most 2^31 - 1 workgroups of 256 rows
static bool rows_ok(long long total) { return total <= 0x7fffffffll * 256; }

}  // namespace omnipq

// bucket ids [b][n] | offsets [b][H + 1] | order [b][n] | sorted xyz [b][n][3] | counters of the CSR build [b][H]
extern "C" long long omnipq_knn_workspace_bytes(int b, int n, int m) {
  if (b < 0 || n < 0 || m < 0) return -1;
  return (long long)b * ((long long)n * 4 + (omnipq::kBqBuckets + 1) * 4ll + (long long)n * 4 + (long long)n * 12 +
                         omnipq::kBqBuckets * 4ll);
}

extern "C" int omnipq_knn(int b, int n, int m, int k, float cell, const float *new_xyz, const float *xyz, int *idx,
                          float *dist2, void *workspace, void *stream) {
  using namespace omnipq;
  if (!normals_sizes_ok(b, n, k) || m < 0 || !(cell > 0.f) || !(cell < __builtin_inff())) return OMNIPQ_EINVAL;
  if (b == 0 || m == 0) return OMNIPQ_OK;
  if (!new_xyz || !idx || (n > 0 && (!xyz || !workspace))) return OMNIPQ_EINVAL;
  const long long rows = (long long)b * m;
  if (!rows_ok(rows * k) || !rows_ok((long long)b * n)) return OMNIPQ_ETOOLARGE;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    knn_empty_kernel<<<blocks_for(rows * k), 256, 0, st>>>(rows * k, idx, dist2);
    OMNIPQ_LAUNCH_CHECK();
    return OMNIPQ_OK;
  }
  int *bucket = (int *)workspace;
  int *offsets = bucket + (size_t)b * n;
  int *order = offsets + (size_t)b * (kBqBuckets + 1);
  float *sorted = (float *)(order + (size_t)b * n);
  int *scratch = (int *)(sorted + (size_t)b * n * 3);
  const float inv_h = 1.0f / cell;
  const long long total = (long long)b * n;
  bq_cell_kernel<<<blocks_for(total), 256, 0, st>>>(total, inv_h, xyz, bucket);
  OMNIPQ_LAUNCH_CHECK();
  const int rc = omnipq_sa_build_csr(b, kBqBuckets, n, 1, bucket, offsets, order, scratch, nullptr, stream);
  if (rc) return rc;
  bq_sorted_xyz_kernel<<<blocks_for(total), 256, 0, st>>>(total, n, xyz, order, sorted);
  OMNIPQ_LAUNCH_CHECK();
  dim3 grid((unsigned)((m + 3) / 4), (unsigned)b);
  knn_kernel<<<grid, 256, 0, st>>>(n, m, k, cell, inv_h, new_xyz, xyz, sorted, offsets, order, idx, dist2);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_normals_plane_fit(int b, int n, int k, const float *xyz, const int *idx, float *normals_out,
                                        double *eig_out, void *stream) {
  using namespace omnipq;
  if (!normals_sizes_ok(b, n, k)) return OMNIPQ_EINVAL;
  if (b == 0 || n == 0) return OMNIPQ_OK;
  if (!xyz || !idx || !normals_out) return OMNIPQ_EINVAL;
  const long long total = (long long)b * n;
  if (!rows_ok(total)) return OMNIPQ_ETOOLARGE;
  plane_fit_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(total, n, k, xyz, idx, normals_out, eig_out);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_normals_smooth(int b, int n, int k, const int *idx, const float *normals_in, float *normals_out,
                                     void *stream) {
  using namespace omnipq;
  if (!normals_sizes_ok(b, n, k)) return OMNIPQ_EINVAL;
  if (b == 0 || n == 0) return OMNIPQ_OK;
  if (!idx || !normals_in || !normals_out || normals_in == normals_out) return OMNIPQ_EINVAL;
  const long long total = (long long)b * n;
  if (!rows_ok(total)) return OMNIPQ_ETOOLARGE;
  smooth_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(total, n, k, idx, normals_in, normals_out);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

extern "C" int omnipq_normals_orient(int b, int n, const float *xyz, const double *centre, float *normals, void *stream) {
  using namespace omnipq;
  if (b < 0 || n < 0 || b > 65535) return OMNIPQ_EINVAL;
  if (b == 0 || n == 0) return OMNIPQ_OK;
  if (!xyz || !centre || !normals) return OMNIPQ_EINVAL;
  const long long total = (long long)b * n;
  if (!rows_ok(total)) return OMNIPQ_ETOOLARGE;
  orient_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(total, n, xyz, centre, normals);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}

// the k-NN workspace | idx [b][n][k] | the second normals buffer [b][n][3]
extern "C" long long omnipq_estimate_normals_workspace_bytes(int b, int n, int k) {
  if (!omnipq::normals_sizes_ok(b, n, k)) return -1;
  return omnipq_knn_workspace_bytes(b, n, n) + (long long)b * n * k * 4 + (long long)b * n * 12;
}

extern "C" int omnipq_estimate_normals(int b, int n, int k, int iters, float cell, const float *xyz, const double *centre,
                                       float *normals_out, void *workspace, void *stream) {
  using namespace omnipq;
  if (!normals_sizes_ok(b, n, k) || iters < 0 || !(cell > 0.f) || !(cell < __builtin_inff())) return OMNIPQ_EINVAL;
  if (b == 0 || n == 0) return OMNIPQ_OK;
  if (!xyz || !centre || !normals_out || !workspace) return OMNIPQ_EINVAL;
  int *idx = (int *)((char *)workspace + omnipq_knn_workspace_bytes(b, n, n));
  float *other = (float *)(idx + (size_t)b * n * k);
  int rc = omnipq_knn(b, n, n, k, cell, xyz, xyz, idx, nullptr, workspace, stream);
  if (rc) return rc;
  // ping-pong so that the last step writes normals_out
  float *cur = (iters % 2) ? other : normals_out, *nxt = (iters % 2) ? normals_out : other;
  rc = omnipq_normals_plane_fit(b, n, k, xyz, idx, cur, nullptr, stream);
  for (int it = 0; it < iters && !rc; ++it) {
    rc = omnipq_normals_smooth(b, n, k, idx, cur, nxt, stream);
    float *t = cur;
    cur = nxt;
    nxt = t;
  }
  if (rc) return rc;
  return omnipq_normals_orient(b, n, xyz, centre, normals_out, stream);
}
