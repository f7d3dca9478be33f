// Inference set-abstraction stage in ONE launch (include/omnipq_sa.h: omnipq_sa_infer): gather -> up to three
// conv1x1 + folded BatchNorm + ReLU layers -> max-pool over every ball, forward only.  In eval mode BatchNorm is the affine
// a = gamma / sqrt(running_var + eps), b = beta - running_mean a, known before the launch, so nothing ties a layer's GEMM to a
// grid-wide reduction and a tile of balls goes from point indices to pooled features without leaving the CU: nothing of shape
// [b m s][.] touches HBM.  Replaces, for `model.eval()` under `torch.no_grad()`, what the reference runs as
// QueryAndGroup + SharedMLP + max_pool2d (pointnet2_modules.py:243-262, pytorch_utils.py:11-64).
//
// Workgroup program (256 threads, persistent over tiles of TR = 64 rows, 128 when nsample == 128, i.e. TR / nsample whole balls):
//   gather   the tile's rows [features | (xyz - centre) / r | 0] into LDS buffer A, 16 bytes per lane, exactly the values
//            omnipq_sa_gather stores (rows past the last ball: zeros)
//   hidden   per layer below the last: a wave owns 64 (or a last 32) output channels for ALL rows of the tile and computes the
//            TRANSPOSED product  W (channels x K) . X^T (K x rows)  -- W fragments from global memory / L2 (every weight is read
//            once per workgroup and tile), X fragments from LDS -- so that a lane holds four consecutive channels of one row in
//            four consecutive accumulator registers: relu(a acc + b) is rounded to e16 once and stored with 8-byte LDS writes into
//            the other buffer
//   last     the same fragments with the operands swapped (X . W^T): a lane holds ONE channel and 16 rows of a 32-row block in its
//            registers, the other lane half the other 16, so the ball maximum is 15 v_max in registers and one exchange between
//            the lane halves; out_f32 / out_pm are written with 128-byte rows.  No atomics: bit-reproducible.
// LDS: a | b of every layer (f32), buffer A = TR x (max(kpad, C_1 when there are three layers) + 8), buffer B = TR x (C_0 + 8)
// (only with two or more layers); + 8 elements = 16 bytes per row keeps the 16-byte fragment reads of 32 consecutive rows off
// each other's banks.  omnipq_sa_infer_lds_bytes states the sum; a shape whose sum exceeds the CU's 160 KiB is refused.
#include <stddef.h>

#include "infer_tiles.h"      // infer_block_gemm, infer_hidden and the chains' constants: shared with csrc/rows_infer.hip

namespace omnipq {

struct InferLayer {
  const e16_t *W;
  int ldw, C, K;
  const float *gamma, *beta, *mean, *var;
  float eps;
};

struct InferArgs {
  int n, m, s, cin, kpad, nlayers, tiles, pitch_a, pitch_b, sum_c;
  float inv_r;
  long long balls;
  const float *xyz, *new_xyz;
  const int *idx;
  const e16_t *feat;
  float *out_f32;
  e16_t *out_pm;
  InferLayer lay[kInferMaxLayers];
};

// the last layer's channels [c0, c0 + 32 NCB): the maximum over every ball of the tile, f32 and its e16 rounding
template <int RB, int NCB>
__device__ __forceinline__ void infer_last(const InferLayer &L, int c0, const float *a, const float *b, const e16_t *Xin,
                                           int pitch_in, int s, long long ball0, long long balls, float *__restrict__ out_f32,
                                           e16_t *__restrict__ out_pm) {
  omnipq_f32x16 acc[NCB][RB];
  infer_block_gemm<RB, NCB, false>(L.W, L.ldw, L.K, c0, Xin, pitch_in, acc);
  const int lane = lane_id(), r = lane & 31, h = lane >> 5;
  const int per = s >> 4;                                   // 16-row groups per ball
#pragma unroll
  for (int j = 0; j < NCB; ++j) {
    const int c = c0 + 32 * j + r;
    const float ac = a[c], bc = b[c];
    float m16[2 * RB];                                      // maxima of rows 16 t .. 16 t + 15 of the tile
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      // register i holds row (i & 3) + 8 (i >> 2) + 4 h of the block: 0 .. 7 the first sixteen rows, 8 .. 15 the second
      float lo = 0.f, hi = 0.f;                             // relu(.) >= 0
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        lo = fmaxf(lo, ac * acc[j][rb][i] + bc);
        hi = fmaxf(hi, ac * acc[j][rb][8 + i] + bc);
      }
      m16[2 * rb] = fmaxf(lo, __shfl_xor(lo, 32));
      m16[2 * rb + 1] = fmaxf(hi, __shfl_xor(hi, 32));
    }
    if (h == 0) {
#pragma unroll
      for (int t0 = 0; t0 < 2 * RB; ++t0) {
        if (t0 % per) continue;
        float v = m16[t0];
#pragma unroll
        for (int t = 1; t < 2 * RB; ++t)
          if (t < per && t0 + t < 2 * RB) v = fmaxf(v, m16[t0 + t]);
        const long long ball = ball0 + t0 / per;
        if (ball < balls) {
          out_f32[(size_t)ball * L.C + c] = v;
          out_pm[(size_t)ball * L.C + c] = (e16_t)v;
        }
      }
    }
  }
}

template <int RB>
__global__ __launch_bounds__(256) void sa_infer_kernel(const InferArgs g) {
  constexpr int TR = 32 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char infer_smem[];
  float *ab = reinterpret_cast<float *>(infer_smem);                       // per layer: a[C] | b[C]
  e16_t *buf_a = reinterpret_cast<e16_t *>(infer_smem + 8 * (size_t)g.sum_c);
  e16_t *buf_b = buf_a + TR * g.pitch_a;
  const int tid = (int)threadIdx.x, wave = tid >> 6;

  // the folded BatchNorm of every layer, f32: a = gamma / sqrt(var + eps), b = beta - mean a
  {
    int off = 0;
    for (int l = 0; l < g.nlayers; ++l) {
      const InferLayer &L = g.lay[l];
      for (int c = tid; c < L.C; c += 256) {
        const float a = L.gamma[c] / sqrtf(L.var[c] + L.eps);
        ab[off + c] = a;
        ab[off + L.C + c] = L.beta[c] - L.mean[c] * a;
      }
      off += 2 * L.C;
    }
  }

  const long long P = g.balls * g.s;
  const int cpr = g.kpad >> 3;                  // 16-byte pieces per gathered row
  for (int tile = (int)blockIdx.x; tile < g.tiles; tile += (int)gridDim.x) {
    __syncthreads();                            // a | b written; the previous tile's last layer has read its operand
    const long long p0 = (long long)tile * TR;
    for (int q = tid; q < TR * cpr; q += 256) {
      const int row = q / cpr, c8 = q - row * cpr;
      const long long p = p0 + row;
      uint4 out = make_uint4(0, 0, 0, 0);
      if (p < P) {
        const long long bm = p / g.s;
        const long long b = bm / g.m;
        const int k = g.idx[p];
        if (c8 * 8 < g.cin) {
          out = *reinterpret_cast<const uint4 *>(g.feat + ((size_t)b * g.n + k) * g.cin + c8 * 8);
        } else if (c8 * 8 == g.cin) {           // subtracted, then multiplied, in f32: the values omnipq_sa_gather stores
          const float *pk = g.xyz + ((size_t)b * g.n + k) * 3;
          const float *pc = g.new_xyz + (size_t)bm * 3;
          out.x = pack_e16x2((pk[0] - pc[0]) * g.inv_r, (pk[1] - pc[1]) * g.inv_r);
          out.y = pack_e16x2((pk[2] - pc[2]) * g.inv_r, 0.f);
        }
      }
      *reinterpret_cast<uint4 *>(buf_a + row * g.pitch_a + c8 * 8) = out;
    }
    __syncthreads();
    int off = 0;
    for (int l = 0; l < g.nlayers; ++l) {
      const InferLayer &L = g.lay[l];
      const e16_t *Xin = (l & 1) ? buf_b : buf_a;
      e16_t *Xout = (l & 1) ? buf_a : buf_b;
      const int pitch_in = (l & 1) ? g.pitch_b : g.pitch_a, pitch_out = (l & 1) ? g.pitch_a : g.pitch_b;
      const float *a = ab + off, *b = ab + off + L.C;
      const bool last = l == g.nlayers - 1;
      const long long ball0 = p0 / g.s;
      const int pairs = L.C >> 6;               // 64-channel units, dealt round robin; a last 32 goes to the next wave
      for (int u = wave; u < pairs; u += 4) {
        if (last)
          infer_last<RB, 2>(L, 64 * u, a, b, Xin, pitch_in, g.s, ball0, g.balls, g.out_f32, g.out_pm);
        else
          infer_hidden<RB, 2>(L.W, L.ldw, L.K, 64 * u, a, b, Xin, pitch_in, Xout, pitch_out);
      }
      if ((L.C & 32) && wave == (pairs & 3)) {
        if (last)
          infer_last<RB, 1>(L, 64 * pairs, a, b, Xin, pitch_in, g.s, ball0, g.balls, g.out_f32, g.out_pm);
        else
          infer_hidden<RB, 1>(L.W, L.ldw, L.K, 64 * pairs, a, b, Xin, pitch_in, Xout, pitch_out);
      }
      off += 2 * L.C;
      if (!last) __syncthreads();
    }
  }
}

// rows per tile, LDS pitches (e16 elements) and bytes of a shape; false: a shape the kernel does not take
static bool infer_layout(int s, int kpad, int nlayers, const int *widths, int *tr, int *pitch_a, int *pitch_b, int *sum_c,
                         long long *bytes) {
  if (s != 16 && s != 32 && s != 64 && s != 128) return false;
  if (nlayers < 1 || nlayers > kInferMaxLayers || !widths) return false;
  if (kpad < 32 || (kpad % 32) || kpad > (1 << 16)) return false;
  int sum = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (widths[l] < 32 || (widths[l] % 32) || widths[l] > kInferMaxC) return false;
    sum += widths[l];
  }
  const int rows = s == 128 ? 128 : 64;
  int wa = kpad;
  if (nlayers == 3 && widths[1] > wa) wa = widths[1];
  const int pa = wa + kInferRowPad, pb = nlayers >= 2 ? widths[0] + kInferRowPad : 0;
  const long long total = 8ll * sum + 2ll * rows * (pa + pb);
  if (total > kInferLdsLimit) return false;
  *tr = rows;
  *pitch_a = pa;
  *pitch_b = pb;
  *sum_c = sum;
  *bytes = total;
  return true;
}

template <int RB>
static void infer_launch(const InferArgs &g, int grid, int lds, hipStream_t stream) {
  auto kern = sa_infer_kernel<RB>;
  static const hipError_t prepared = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, kInferLdsLimit);
  (void)prepared;
  kern<<<grid, 256, lds, stream>>>(g);
}

}  // namespace omnipq

using namespace omnipq;

extern "C" const char *omnipq_sa_infer_layer_record(void) {
  static_assert(sizeof(omnipq_sa_infer_layer) == 56 && sizeof(void *) == 8, "omnipq_sa_infer_layer: size");
  static_assert(offsetof(omnipq_sa_infer_layer, W) == 0, "omnipq_sa_infer_layer.W: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, ldw) == 8, "omnipq_sa_infer_layer.ldw: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, C) == 12, "omnipq_sa_infer_layer.C: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, gamma) == 16, "omnipq_sa_infer_layer.gamma: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, beta) == 24, "omnipq_sa_infer_layer.beta: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, running_mean) == 32, "omnipq_sa_infer_layer.running_mean: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, running_var) == 40, "omnipq_sa_infer_layer.running_var: offset");
  static_assert(offsetof(omnipq_sa_infer_layer, eps) == 48, "omnipq_sa_infer_layer.eps: offset");
  return "struct omnipq_sa_infer_layer W:p ldw:i C:i gamma:p beta:p running_mean:p running_var:p eps:f";
}

extern "C" long long omnipq_sa_infer_lds_bytes(int s, int kpad, int nlayers, const int *widths) {
  int tr, pa, pb, sum;
  long long bytes;
  return infer_layout(s, kpad, nlayers, widths, &tr, &pa, &pb, &sum, &bytes) ? bytes : -1;
}

extern "C" int omnipq_sa_infer(int b, int n, int m, int s, int cin, int kpad, float inv_radius, const float *xyz,
                               const float *new_xyz, const int *idx, const void *feat_pm, int nlayers, const void *layers,
                               float *out_f32, void *out_pm, void *stream) {
  if (b < 0 || n <= 0 || m < 0 || cin < 0 || (cin % 8) || kpad < cin + 3) return OMNIPQ_EINVAL;
  if (nlayers < 1 || nlayers > kInferMaxLayers || !layers) return OMNIPQ_EINVAL;
  const omnipq_sa_infer_layer *rec = static_cast<const omnipq_sa_infer_layer *>(layers);
  int widths[kInferMaxLayers];
  for (int l = 0; l < nlayers; ++l) widths[l] = rec[l].C;
  InferArgs g;
  int tr;
  long long bytes;
  if (!infer_layout(s, kpad, nlayers, widths, &tr, &g.pitch_a, &g.pitch_b, &g.sum_c, &bytes)) return OMNIPQ_EINVAL;
  for (int l = 0; l < nlayers; ++l) {
    const int K = l == 0 ? kpad : widths[l - 1];
    if (!rec[l].W || !rec[l].gamma || !rec[l].beta || !rec[l].running_mean || !rec[l].running_var) return OMNIPQ_EINVAL;
    if (rec[l].ldw < K || (rec[l].ldw % 8)) return OMNIPQ_EINVAL;
    g.lay[l] = InferLayer{(const e16_t *)rec[l].W, rec[l].ldw, rec[l].C, K, rec[l].gamma, rec[l].beta, rec[l].running_mean,
                          rec[l].running_var, rec[l].eps};
  }
  if (!xyz || !new_xyz || !idx || !out_f32 || !out_pm || (cin > 0 && !feat_pm)) return OMNIPQ_EINVAL;
  const long long balls = (long long)b * m;
  const long long tiles = (balls * s + tr - 1) / tr;
  if (tiles > 0x7fffffffll) return OMNIPQ_ETOOLARGE;
  if (balls == 0) return OMNIPQ_OK;
  g.n = n;
  g.m = m;
  g.s = s;
  g.cin = cin;
  g.kpad = kpad;
  g.nlayers = nlayers;
  g.tiles = (int)tiles;
  g.inv_r = inv_radius;
  g.balls = balls;
  g.xyz = xyz;
  g.new_xyz = new_xyz;
  g.idx = idx;
  g.feat = (const e16_t *)feat_pm;
  g.out_f32 = out_f32;
  g.out_pm = (e16_t *)out_pm;
  // persistent workgroups: as many as stay resident (LDS; two waves per SIMD at the kernel's ~200 registers), static for a
  // given shape
  long long per_cu = kInferLdsLimit / bytes;
  if (per_cu > 2) per_cu = 2;
  long long grid = per_cu * infer_cus();
  if (grid > tiles) grid = tiles;
  if (tr == 128)
    infer_launch<4>(g, (int)grid, (int)bytes, (hipStream_t)stream);
  else
    infer_launch<2>(g, (int)grid, (int)bytes, (hipStream_t)stream);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
