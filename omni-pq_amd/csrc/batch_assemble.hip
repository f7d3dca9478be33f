// Device-resident scenes -> one training batch: draw, gather, augment, instance extents, votes, box and quad labels.
// Contract, arithmetic and launch list: include/omnipq_data.h.  Compiled with -ffp-contract=off: every multiply and add
// below is rounded on its own, which is what makes the points bit-equal to the host arithmetic they restate.
#include "common.h"
#include "omnipq_data.h"

namespace omnipq {
namespace {

constexpr int kAsmThreads = 256;
constexpr int kAsmPerThread = 4;                                // positions per thread of the points kernel
constexpr int kAsmTile = kAsmThreads * kAsmPerThread;           // positions per workgroup
constexpr int kExtWords = 8;                                    // min xyz, max xyz, first position, spare
constexpr int kMaxInst = OMNIPQ_ASM_MAX_INSTANCES;
constexpr int kMaxObj = OMNIPQ_ASM_MAX_OBJ;
constexpr int kMaxQuad = OMNIPQ_ASM_MAX_QUAD;
constexpr int kProp = OMNIPQ_ASM_NUM_PROPOSAL;

// workspace per item: extents u32 [1024][8], instance records f32 [1024][4] (centre, ilabel as int bits), centres f64 [64][3]
constexpr long long kWsExtBytes = (long long)kMaxInst * kExtWords * 4;
constexpr long long kWsInstBytes = (long long)kMaxInst * 4 * 4;
constexpr long long kWsGtcBytes = (long long)kMaxObj * 3 * 8;
constexpr long long kWsItemBytes = kWsExtBytes + kWsInstBytes + kWsGtcBytes;

struct Ws {
  unsigned *ext;
  float *inst;
  double *gtc;
};
__host__ __device__ inline Ws ws_of(void *workspace, int b) {
  char *p = (char *)workspace;
  Ws w;
  w.ext = (unsigned *)p;
  w.inst = (float *)(p + kWsExtBytes * b);
  w.gtc = (double *)(p + (kWsExtBytes + kWsInstBytes) * b);
  return w;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned fmix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

struct DrawKey {
  unsigned rk[OMNIPQ_ASM_ROUNDS];
};
__device__ __forceinline__ DrawKey draw_key(unsigned long long seed, int stream_id, int slot) {
  const unsigned long long key = mix64(seed ^ mix64((((unsigned long long)stream_id << 32) | (unsigned)slot) + 1ull));
  DrawKey k;
#pragma unroll
  for (int r = 0; r < OMNIPQ_ASM_ROUNDS; ++r) k.rk[r] = (unsigned)mix64(key + (unsigned long long)r);
  return k;
}
// n >= 1.  without: position p < n of a permutation of [0, n); else uniform with replacement.
__device__ __forceinline__ int draw_index(const DrawKey &k, unsigned p, unsigned n, bool without, int h) {
  if (!without) {
    const unsigned u = fmix32(fmix32(p ^ k.rk[0]) ^ k.rk[1]);
    return (int)(((unsigned long long)u * n) >> 32);
  }
  const unsigned mask = (1u << h) - 1u;
  unsigned x = p;
  do {                                          // cycle walking: x started inside [0, n), so its cycle returns there
    unsigned L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < OMNIPQ_ASM_ROUNDS; ++r) {
      const unsigned t = L ^ (fmix32(R ^ k.rk[r]) & mask);
      L = R;
      R = t;
    }
    x = (L << h) | R;
  } while (x >= n);
  return (int)x;
}
__device__ __forceinline__ int half_bits(unsigned n) {
  int h = 1;
  while (h < 16 && (1ull << (2 * h)) < (unsigned long long)n) ++h;
  return h;
}

// order-preserving f32 -> u32
__device__ __forceinline__ unsigned enc_f32(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_f32(unsigned e) {
  const unsigned u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  return __builtin_bit_cast(float, u);
}

struct Scene {
  long long off;
  int n, ninst, nbox, nrect, total_quads, nh, slot;
};
// the table entry of the scene behind item s, bounded by the arena: anything out of range is an empty scene
__device__ __forceinline__ Scene scene_of(const omnipq_asm_bank &bk, const int *scene_slot, int s) {
  Scene sc = {0, 0, 0, 0, 0, 0, 0, scene_slot[s]};
  if (sc.slot < 0 || sc.slot >= bk.scenes) return sc;
  const int *m = bk.meta + (long long)sc.slot * OMNIPQ_ASM_META_INTS;
  const long long off = bk.row_offset[sc.slot];
  const int n = m[0];
  if (off < 0 || n < 0 || off + n > bk.rows_total) return sc;
  sc.off = off;
  sc.n = n;
  sc.ninst = min(max(m[1], 0), kMaxInst);
  sc.nbox = min(max(m[2], 0), kMaxObj);
  sc.nrect = min(max(m[3], 0), kMaxQuad);
  sc.total_quads = m[4];
  sc.nh = min(max(m[5], 0), OMNIPQ_ASM_MAX_HQUAD);
  return sc;
}

struct Aug {
  bool fx, fy, ident;               // ident: no flip, R = I, scale = 1 -- the rows are copied, as the reference leaves them
  double r[9], scale;
};
__device__ __forceinline__ Aug aug_of(const double *params, int s) {
  const double *p = params + (long long)s * OMNIPQ_ASM_PARAM_DOUBLES;
  Aug a;
  a.fx = p[0] != 0.0;
  a.fy = p[1] != 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) a.r[i] = p[2 + i];
  a.scale = p[11];
  a.ident = !a.fx && !a.fy && a.scale == 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) a.ident = a.ident && a.r[i] == ((i % 4 == 0) ? 1.0 : 0.0);
  return a;
}
// v <- R v in f64 with all three columns (boxes, quads)
__device__ __forceinline__ void rot3(const Aug &a, double &x, double &y, double &z) {
  const double nx = x * a.r[0] + y * a.r[1] + z * a.r[2];
  const double ny = x * a.r[3] + y * a.r[4] + z * a.r[5];
  const double nz = x * a.r[6] + y * a.r[7] + z * a.r[8];
  x = nx;
  y = ny;
  z = nz;
}

// ---- launch 1: labels and scalars of every item, f64 box centres, reset of the extent table ---------------------------
__global__ __launch_bounds__(kAsmThreads) void asm_labels_kernel(omnipq_asm_bank bk, omnipq_asm_batch bt, omnipq_asm_out o,
                                                                  void *workspace) {
  const int s = blockIdx.x, t = threadIdx.x;
  const Scene sc = scene_of(bk, bt.scene_slot, s);
  const Aug a = aug_of(bt.params, s);
  const Ws w = ws_of(workspace, bt.b);
  const double *lab = bk.labels + (long long)max(min(sc.slot, bk.scenes - 1), 0) * OMNIPQ_ASM_LABEL_DOUBLES;

  if (bt.flavour == 0) {
    unsigned *ext = w.ext + (long long)s * kMaxInst * kExtWords;
    for (int i = t; i < kMaxInst * kExtWords; i += kAsmThreads) {
      const int word = i % kExtWords;
      ext[i] = (word >= 3 && word < 6) ? 0u : 0xFFFFFFFFu;      // max words start at the bottom, min words and `first` at the top
    }
  }
  if (t < kMaxObj) {
    const int j = t;
    const bool real = j < sc.nbox;
    double c[3] = {0, 0, 0}, l[3] = {0, 0, 0};
    int cls = 0;
    if (real) {
      const double *bx = lab + j * 7;
      c[0] = bx[0], c[1] = bx[1], c[2] = bx[2], l[0] = bx[3], l[1] = bx[4], l[2] = bx[5];
      cls = (int)bx[6];
    }
    if (a.fx) c[0] = -1.0 * c[0];
    if (a.fy) c[1] = -1.0 * c[1];
    rot3(a, c[0], c[1], c[2]);
    const double dx = l[0] / 2.0, dy = l[1] / 2.0;
    double mx = 0, my = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double sx = (q == 1 || q == 2) ? 1.0 : -1.0, sy = (q >= 2) ? 1.0 : -1.0;
      double px = sx * dx, py = sy * dy, pz = 0.0;
      rot3(a, px, py, pz);
      mx = q == 0 ? px : fmax(mx, px);
      my = q == 0 ? py : fmax(my, py);
    }
    l[0] = 2.0 * mx;
    l[1] = 2.0 * my;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c[d] *= a.scale;
      l[d] *= a.scale;
    }
    const long long row = (long long)s * kMaxObj + j;
    if (bt.flavour == 0) {
      if (!real)
        for (int d = 0; d < 3; ++d) c[d] += 1000.0;
      for (int d = 0; d < 3; ++d) w.gtc[row * 3 + d] = c[d];
      if (bt.n_sizes > 0) cls = min(max(cls, 0), bt.n_sizes - 1);
      for (int d = 0; d < 3; ++d) {
        o.size_gts[row * 3 + d] = real ? (float)l[d] : 0.f;
        o.size_residual_label[row * 3 + d] = real ? (float)(l[d] - bt.mean_size[cls * 3 + d]) : 0.f;
      }
      o.size_class_label[row] = real ? cls : 0;
      o.sem_cls_label[row] = real ? cls : 0;
      o.box_label_mask[row] = real ? 1.f : 0.f;
    } else {
      for (int d = 0; d < 3; ++d) o.size_label[row * 3 + d] = (float)l[d];
    }
    for (int d = 0; d < 3; ++d) o.center_label[row * 3 + d] = (float)c[d];
    o.heading_class_label[row] = 0;
    o.heading_residual_label[row] = 0.f;
  } else if (bt.flavour == 0 && t < kMaxObj + kMaxQuad) {
    const int j = t - kMaxObj;
    const bool real = j < sc.nrect;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (real) {
      const double *q = lab + kMaxObj * 7 + j * 8;
      for (int d = 0; d < 8; ++d) v[d] = q[d];
      if (a.fx) v[0] = -1.0 * v[0], v[3] = -1.0 * v[3];
      if (a.fy) v[1] = -1.0 * v[1], v[4] = -1.0 * v[4];
      rot3(a, v[0], v[1], v[2]);
      rot3(a, v[3], v[4], v[5]);
      v[0] *= a.scale, v[1] *= a.scale, v[2] *= a.scale, v[6] *= a.scale, v[7] *= a.scale;
    }
    const long long row = (long long)s * kMaxQuad + j;
    for (int d = 0; d < 3; ++d) {
      o.gt_quad_centers[row * 3 + d] = (float)v[d];
      o.gt_normal_vectors[row * 3 + d] = (float)v[3 + d];
    }
    o.gt_quad_sizes[row * 2] = (float)v[6];
    o.gt_quad_sizes[row * 2 + 1] = (float)v[7];
  } else if (bt.flavour == 0 && t < kMaxObj + kMaxQuad + 16) {
    const int j = t - kMaxObj - kMaxQuad;              // corner j % 4 of horizontal quad j / 4
    double v[3] = {0, 0, 0};
    if (j / 4 < sc.nh) {
      const double *q = lab + kMaxObj * 7 + kMaxQuad * 8 + j * 3;
      v[0] = q[0], v[1] = q[1], v[2] = q[2];
      if (a.fx) v[0] = -1.0 * v[0];
      if (a.fy) v[1] = -1.0 * v[1];
      rot3(a, v[0], v[1], v[2]);
      v[0] *= a.scale, v[1] *= a.scale, v[2] *= a.scale;
    }
    for (int d = 0; d < 3; ++d) o.horizontal_quads[((long long)s * 16 + j) * 3 + d] = (float)v[d];
  } else if (t == kAsmThreads - 1) {
    if (bt.flavour == 0) {
      o.flip_x_axis[s] = a.fx ? 1 : 0;
      o.flip_y_axis[s] = a.fy ? 1 : 0;
      o.scan_idx[s] = sc.slot;
    } else {
      o.flip_x_axis[s] = (a.fx && !a.fy) ? 1 : 0;
      o.flip_y_axis[s] = 0;
    }
    for (int i = 0; i < 9; ++i) o.rot_mat[(long long)s * 9 + i] = (float)a.r[i];
    o.scale[s] = (float)a.scale;
  }
  for (int i = t; i < kProp; i += kAsmThreads) {
    o.num_gt_boxes[(long long)s * kProp + i] = sc.nbox;
    if (bt.flavour == 0) {
      o.num_gt_quads[(long long)s * kProp + i] = sc.nrect;
      o.num_total_quads[(long long)s * kProp + i] = sc.total_quads;
    }
  }
}

// ---- launch 2: draw, gather, augment, extents ---------------------------------------------------------------------------
// EXT: the labelled flavour, whose workgroups fold the instance extents in LDS; the unlabelled one carries none
template <bool EXT>
__global__ __launch_bounds__(kAsmThreads) void asm_points_kernel(omnipq_asm_bank bk, omnipq_asm_batch bt, omnipq_asm_out o,
                                                                  void *workspace) {
  __shared__ unsigned lds[EXT ? kMaxInst * 7 : 1];
  const int s = blockIdx.y, t = threadIdx.x;
  const Scene sc = scene_of(bk, bt.scene_slot, s);
  const int k = bt.k, pitch = bk.pitch;
  const bool extents = EXT && sc.ninst > 0;
  const Aug a = aug_of(bt.params, s);
  const float fscale = (float)a.scale;
  // the teacher's rows of this tile first (draw, gather), then the student's
  {
    const int *supplied = bt.ema_choices_in;
    DrawKey key = {};
    int h = 1;
    if (!supplied && sc.n > 0) {
      key = draw_key(*bt.seed, 1, s);
      h = half_bits((unsigned)sc.n);
    }
    for (int j = 0; j < kAsmPerThread; ++j) {
      const int p = blockIdx.x * kAsmTile + j * kAsmThreads + t;
      if (p >= k) break;
      const long long at = (long long)s * k + p;
      const int idx = supplied ? supplied[at] : (sc.n > 0 ? draw_index(key, (unsigned)p, (unsigned)sc.n, sc.n >= k, h) : -1);
      o.ema_choices[at] = idx;
      const bool ok = idx >= 0 && idx < sc.n;
      const long long row = sc.off + (ok ? idx : 0);
      for (int c = 0; c < pitch; ++c) o.ema_point_clouds[at * pitch + c] = ok ? bk.points[row * pitch + c] : 0.f;
    }
  }
  if (extents) {
    for (int i = t; i < sc.ninst * 7; i += kAsmThreads) lds[i] = (i % 7 >= 3 && i % 7 < 6) ? 0u : 0xFFFFFFFFu;
    __syncthreads();
  }
  const int *supplied = bt.choices_in;
  DrawKey key = {};
  int h = 1;
  if (!supplied && sc.n > 0) {
    key = draw_key(*bt.seed, 0, s);
    h = half_bits((unsigned)sc.n);
  }
  int *idx_out = o.choices;
  float *pts_out = o.point_clouds;

  for (int j = 0; j < kAsmPerThread; ++j) {
    const int p = blockIdx.x * kAsmTile + j * kAsmThreads + t;
    if (p >= k) break;
    const long long at = (long long)s * k + p;
    int idx;
    if (supplied)
      idx = supplied[at];
    else
      idx = sc.n > 0 ? draw_index(key, (unsigned)p, (unsigned)sc.n, sc.n >= k, h) : -1;
    idx_out[at] = idx;
    const bool ok = idx >= 0 && idx < sc.n;
    const long long row = sc.off + (ok ? idx : 0);
    float v[OMNIPQ_ASM_MAX_PITCH];
#pragma unroll
    for (int c = 0; c < OMNIPQ_ASM_MAX_PITCH; ++c) v[c] = (ok && c < pitch) ? bk.points[row * pitch + c] : 0.f;
    float nrm[3];
    for (int c = 0; c < 3; ++c) nrm[c] = ok ? bk.normals[row * 3 + c] : 0.f;
    if (ok && !a.ident) {
      if (a.fx) v[0] = -v[0];
      if (a.fy) v[1] = -v[1];
      const float x = (float)((double)v[0] * a.r[0] + (double)v[1] * a.r[1]);
      const float y = (float)((double)v[0] * a.r[3] + (double)v[1] * a.r[4]);
      v[0] = x * fscale;
      v[1] = y * fscale;
      v[2] = v[2] * fscale;
      if (bt.flavour == 0) {
        if (a.fx) nrm[0] = -nrm[0];
        if (a.fy) nrm[1] = -nrm[1];
        const float nx = (float)((double)nrm[0] * a.r[0] + (double)nrm[1] * a.r[1]);
        const float ny = (float)((double)nrm[0] * a.r[3] + (double)nrm[1] * a.r[4]);
        nrm[0] = nx;
        nrm[1] = ny;
      }
    }
#pragma unroll
    for (int c = 0; c < OMNIPQ_ASM_MAX_PITCH; ++c)
      if (c < pitch) pts_out[at * pitch + c] = (ok && !a.ident && c == bk.height_col) ? v[c] * fscale : v[c];
    for (int c = 0; c < 3; ++c) o.vertex_normals[at * 3 + c] = nrm[c];
    if (bt.flavour == 0) {
      o.semantic_labels[at] = ok ? (float)bk.semantic[row] : 0.f;
      if (o.pcl_color)
        for (int c = 0; c < 3; ++c) o.pcl_color[at * 3 + c] = (ok && bk.colors) ? bk.colors[row * 3 + c] : 0.f;
      if (extents && ok) {
        const int g = bk.instance[row];
        if (g >= 0 && g < sc.ninst) {
          unsigned *e = lds + g * 7;
          for (int c = 0; c < 3; ++c) {
            const unsigned enc = enc_f32(v[c]);
            atomicMin(e + c, enc);
            atomicMax(e + 3 + c, enc);
          }
          atomicMin(e + 6, (unsigned)p);
        }
      }
    }
  }
  if (extents) {
    __syncthreads();
    unsigned *ext = ws_of(workspace, bt.b).ext + (long long)s * kMaxInst * kExtWords;
    for (int g = t; g < sc.ninst; g += kAsmThreads) {
      const unsigned *e = lds + g * 7;
      if (e[6] == 0xFFFFFFFFu) continue;               // this workgroup sampled no point of the instance
      unsigned *dst = ext + g * kExtWords;
      for (int c = 0; c < 3; ++c) {
        atomicMin(dst + c, e[c]);
        atomicMax(dst + 3 + c, e[3 + c]);
      }
      atomicMin(dst + 6, e[6]);
    }
  }
}

// ---- launch 3: centre, validity and nearest box of every instance -------------------------------------------------------
__global__ __launch_bounds__(kAsmThreads) void asm_instance_kernel(omnipq_asm_bank bk, omnipq_asm_batch bt, omnipq_asm_out o,
                                                                    void *workspace) {
  __shared__ double gtc[kMaxObj * 3];
  const int s = blockIdx.x, t = threadIdx.x;
  const Scene sc = scene_of(bk, bt.scene_slot, s);
  const Ws w = ws_of(workspace, bt.b);
  if (t < kMaxObj * 3) gtc[t] = w.gtc[(long long)s * kMaxObj * 3 + t];
  __syncthreads();
  const unsigned *ext = w.ext + (long long)s * kMaxInst * kExtWords;
  float *inst = w.inst + (long long)s * kMaxInst * 4;
  for (int g = t; g < sc.ninst; g += kAsmThreads) {
    const unsigned *e = ext + g * kExtWords;
    float c[3] = {0.f, 0.f, 0.f};
    int ilabel = -1;
    const unsigned first = e[6];
    if (first != 0xFFFFFFFFu && first < (unsigned)bt.k) {
      const int idx = o.choices[(long long)s * bt.k + first];
      bool valid = false;
      if (idx >= 0 && idx < sc.n) {
        const int sem = bk.semantic[sc.off + idx];
        for (int i = 0; i < bt.n_ids; ++i) valid |= bt.nyu40ids[i] == sem;
      }
      if (valid) {
        for (int d = 0; d < 3; ++d) c[d] = 0.5f * (dec_f32(e[d]) + dec_f32(e[3 + d]));
        double best = 0.0;
        for (int j = 0; j < kMaxObj; ++j) {
          const double d0 = (double)c[0] - gtc[j * 3], d1 = (double)c[1] - gtc[j * 3 + 1], d2 = (double)c[2] - gtc[j * 3 + 2];
          const double dist = d0 * d0 + d1 * d1 + d2 * d2;
          if (j == 0 || dist < best) {
            best = dist;
            ilabel = j;
          }
        }
      }
    }
    inst[g * 4] = c[0];
    inst[g * 4 + 1] = c[1];
    inst[g * 4 + 2] = c[2];
    inst[g * 4 + 3] = __builtin_bit_cast(float, ilabel);
  }
}

// ---- launch 4: votes ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAsmThreads) void asm_votes_kernel(omnipq_asm_bank bk, omnipq_asm_batch bt, omnipq_asm_out o,
                                                                 void *workspace) {
  const int s = blockIdx.y;
  const int p = blockIdx.x * kAsmThreads + threadIdx.x;
  if (p >= bt.k) return;
  const Scene sc = scene_of(bk, bt.scene_slot, s);
  const long long at = (long long)s * bt.k + p;
  const int idx = o.choices[at];
  float vote[3] = {0.f, 0.f, 0.f};
  long long mask = 0, label = -1;
  if (idx >= 0 && idx < sc.n) {
    const int g = bk.instance[sc.off + idx];
    if (g >= 0 && g < sc.ninst) {
      const float *rec = ws_of(workspace, bt.b).inst + ((long long)s * kMaxInst + g) * 4;
      const int ilabel = __builtin_bit_cast(int, rec[3]);
      if (ilabel >= 0) {
        for (int d = 0; d < 3; ++d) vote[d] = rec[d] - o.point_clouds[at * bk.pitch + d];
        mask = 1;
        label = ilabel;
      }
    }
  }
  for (int r = 0; r < 3; ++r)
    for (int d = 0; d < 3; ++d) o.vote_label[at * 9 + r * 3 + d] = vote[d];
  o.vote_label_mask[at] = mask;
  o.point_instance_label[at] = label;
}

}  // namespace
}  // namespace omnipq

extern "C" long long omnipq_assemble_workspace_bytes(int b) {
  if (b < 1 || b > OMNIPQ_ASM_MAX_BATCH) return 0;
  return omnipq::kWsItemBytes * b;
}

extern "C" int omnipq_assemble_batch(const omnipq_asm_bank *bank, const omnipq_asm_batch *batch, const omnipq_asm_out *out,
                                     void *workspace, void *stream) {
  if (!bank || !batch || !out) return OMNIPQ_EINVAL;
  const omnipq_asm_bank &bk = *bank;
  const omnipq_asm_batch &bt = *batch;
  const omnipq_asm_out &o = *out;
  if (bt.b < 0 || bt.k < 1 || bk.scenes < 1 || bk.pitch < 3 || bk.rows_total < 0) return OMNIPQ_EINVAL;
  if (bt.flavour != 0 && bt.flavour != 1) return OMNIPQ_EINVAL;
  if (bt.n_ids < 0 || (bt.flavour == 0 && bt.n_sizes < 1)) return OMNIPQ_EINVAL;
  if (bt.b > OMNIPQ_ASM_MAX_BATCH || bt.k > OMNIPQ_ASM_MAX_K || bk.pitch > OMNIPQ_ASM_MAX_PITCH ||
      bt.n_ids > OMNIPQ_ASM_MAX_IDS)
    return OMNIPQ_ETOOLARGE;
  if (bk.height_col != -1 && (bk.height_col < 3 || bk.height_col >= bk.pitch)) return OMNIPQ_EINVAL;
  if (bt.b == 0) return OMNIPQ_OK;
  if (!bk.points || !bk.normals || !bk.row_offset || !bk.meta || !bk.labels || !bt.scene_slot || !bt.params) return OMNIPQ_EINVAL;
  if ((!bt.choices_in || !bt.ema_choices_in) && !bt.seed) return OMNIPQ_EINVAL;
  if (!o.point_clouds || !o.vertex_normals || !o.ema_point_clouds || !o.choices || !o.ema_choices || !o.center_label ||
      !o.heading_class_label || !o.heading_residual_label || !o.num_gt_boxes || !o.flip_x_axis || !o.flip_y_axis ||
      !o.rot_mat || !o.scale)
    return OMNIPQ_EINVAL;
  if (bt.flavour == 0) {
    if (!workspace || !bk.instance || !bk.semantic || !bt.mean_size || (bt.n_ids > 0 && !bt.nyu40ids)) return OMNIPQ_EINVAL;
    if (!o.semantic_labels || !o.vote_label || !o.vote_label_mask || !o.point_instance_label || !o.size_class_label ||
        !o.size_residual_label || !o.size_gts || !o.sem_cls_label || !o.box_label_mask || !o.gt_quad_centers ||
        !o.gt_normal_vectors || !o.gt_quad_sizes || !o.num_gt_quads || !o.num_total_quads || !o.horizontal_quads ||
        !o.scan_idx)
      return OMNIPQ_EINVAL;
  } else if (!o.size_label) {
    return OMNIPQ_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned b = (unsigned)bt.b;
  omnipq::asm_labels_kernel<<<b, omnipq::kAsmThreads, 0, st>>>(bk, bt, o, workspace);
  OMNIPQ_LAUNCH_CHECK();
  const dim3 pgrid((unsigned)((bt.k + omnipq::kAsmTile - 1) / omnipq::kAsmTile), b);
  if (bt.flavour == 0)
    omnipq::asm_points_kernel<true><<<pgrid, omnipq::kAsmThreads, 0, st>>>(bk, bt, o, workspace);
  else
    omnipq::asm_points_kernel<false><<<pgrid, omnipq::kAsmThreads, 0, st>>>(bk, bt, o, workspace);
  OMNIPQ_LAUNCH_CHECK();
  if (bt.flavour == 0) {
    omnipq::asm_instance_kernel<<<b, omnipq::kAsmThreads, 0, st>>>(bk, bt, o, workspace);
    OMNIPQ_LAUNCH_CHECK();
    const dim3 vgrid((unsigned)((bt.k + omnipq::kAsmThreads - 1) / omnipq::kAsmThreads), b);
    omnipq::asm_votes_kernel<<<vgrid, omnipq::kAsmThreads, 0, st>>>(bk, bt, o, workspace);
    OMNIPQ_LAUNCH_CHECK();
  }
  return OMNIPQ_OK;
}
