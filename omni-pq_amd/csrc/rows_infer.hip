// Inference per-point stack in ONE launch (include/omnipq_decoder.h: omnipq_rows_infer): one to three linear
// layers on rows, each followed by a folded BatchNorm + ReLU, a ReLU, or nothing, forward only.  In eval mode BatchNorm is the
// affine a = gamma / sqrt(running_var + eps), b = beta - (running_mean - bias) a, known before the launch, so a tile of rows
// goes from the input to the last layer's output without leaving the CU.  Replaces, for `model.eval()` under
// `torch.no_grad()`, what pointnet2/rows_mlp.py issues per layer on its stored route: omnipq_pad_rows_e16, one NT GEMM, the
// ATen launches that rebuild a | b and omnipq_bnrelu.  It is csrc/sa_infer.hip's chain (infer_tiles.h) without the gather in
// front and without the pool behind.
//
// Workgroup program (256 threads, persistent over tiles of TR = 64 rows; 32 where 64 rows do not fit the CU's LDS):
//   fold     a | b of every layer into LDS, f32, once per workgroup; without BatchNorm a = 1, b = bias (or 0)
//   stage    the tile's rows [x | 0 .. kpad) into LDS buffer A: one rounding to e16, exactly the values omnipq_pad_rows_e16
//            stores; rows past n are zeros and are never read from x
//   layers   every layer, the last one too, as the TRANSPOSED product of infer_hidden: a lane holds four consecutive channels of
//            a row, e16(relu(a acc + b)) (or without relu) goes to the other LDS buffer with 8-byte writes
//   store    the last layer's tile leaves the free buffer in 16-byte pieces of whole rows; rows past n are not written
// No atomics (bit-reproducible), no host read, no allocation, a static grid for a given shape.
// LDS: a | b of every layer (f32), buffer A = TR x (max(kpad, C_1) + 8), buffer B = TR x (max(C_0, C_2) + 8).
#include <stddef.h>

#include "infer_tiles.h"
#include "omnipq_decoder.h"

namespace omnipq {

constexpr int kRowsInferMaxK = 1024;

struct RowsLayer {
  const e16_t *W;
  int ldw, C, K, relu;
  const float *bias, *gamma, *beta, *mean, *var;
  float eps;
};

struct RowsArgs {
  long long n, ldx;
  int cin, kpad, nlayers, tiles, pitch_a, pitch_b, sum_c, x_f32, x_vec;
  const void *x;
  e16_t *out;
  RowsLayer lay[kInferMaxLayers];
};

template <int RB, int NCB>
__device__ __forceinline__ void rows_layer(const RowsLayer &L, int c0, const float *a, const float *b, const e16_t *Xin,
                                           int pitch_in, e16_t *Xout, int pitch_out) {
  if (L.relu)
    infer_hidden<RB, NCB, true>(L.W, L.ldw, L.K, c0, a, b, Xin, pitch_in, Xout, pitch_out);
  else
    infer_hidden<RB, NCB, false>(L.W, L.ldw, L.K, c0, a, b, Xin, pitch_in, Xout, pitch_out);
}

template <int RB>
__global__ __launch_bounds__(256) void rows_infer_kernel(const RowsArgs g) {
  constexpr int TR = 32 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
  float *ab = reinterpret_cast<float *>(rows_smem);                        // per layer: a[C] | b[C]
  e16_t *buf_a = reinterpret_cast<e16_t *>(rows_smem + 8 * (size_t)g.sum_c);
  e16_t *buf_b = buf_a + TR * g.pitch_a;
  const int tid = (int)threadIdx.x, wave = tid >> 6;

  {
    int off = 0;
    for (int l = 0; l < g.nlayers; ++l) {
      const RowsLayer &L = g.lay[l];
      for (int c = tid; c < L.C; c += 256) {
        float a = 1.f, b = L.bias ? L.bias[c] : 0.f;
        if (L.gamma) {                          // a conv bias that feeds a BatchNorm only moves the mean
          a = L.gamma[c] / sqrtf(L.var[c] + L.eps);
          const float mean = L.bias ? L.mean[c] - b : L.mean[c];
          b = L.beta[c] - mean * a;
        }
        ab[off + c] = a;
        ab[off + L.C + c] = b;
      }
      off += 2 * L.C;
    }
  }

  const int cpr = g.kpad >> 3;                  // 16-byte pieces per staged row
  const RowsLayer &last = g.lay[g.nlayers - 1];
  const int opr = last.C >> 3;                  // ... and per output row
  e16_t *Xlast = (g.nlayers & 1) ? buf_b : buf_a;
  const int pitch_last = (g.nlayers & 1) ? g.pitch_b : g.pitch_a;
  for (int tile = (int)blockIdx.x; tile < g.tiles; tile += (int)gridDim.x) {
    __syncthreads();                            // a | b written; the previous tile's rows have left their buffer
    const long long p0 = (long long)tile * TR;
    for (int q = tid; q < TR * cpr; q += 256) {
      const int row = q / cpr, col = (q - row * cpr) * 8;
      const long long p = p0 + row;
      e16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (e16_t)0.f;
      if (p < g.n && col < g.cin) {
        if (g.x_vec && col + 8 <= g.cin) {
          v = infer_load8(reinterpret_cast<const e16_t *>(g.x) + p * g.ldx + col);
        } else if (g.x_f32) {
          const float *xr = reinterpret_cast<const float *>(g.x) + p * g.ldx + col;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (col + j < g.cin) v[j] = (e16_t)xr[j];
        } else {
          const e16_t *xr = reinterpret_cast<const e16_t *>(g.x) + p * g.ldx + col;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (col + j < g.cin) v[j] = xr[j];
        }
      }
      *reinterpret_cast<e16x8 *>(buf_a + row * g.pitch_a + col) = v;
    }
    __syncthreads();
    int off = 0;
    for (int l = 0; l < g.nlayers; ++l) {
      const RowsLayer &L = g.lay[l];
      const e16_t *Xin = (l & 1) ? buf_b : buf_a;
      e16_t *Xout = (l & 1) ? buf_a : buf_b;
      const int pitch_in = (l & 1) ? g.pitch_b : g.pitch_a, pitch_out = (l & 1) ? g.pitch_a : g.pitch_b;
      const float *a = ab + off, *b = ab + off + L.C;
      const int pairs = L.C >> 6;               // 64-channel units, dealt round robin; a last 32 goes to the next wave
      for (int u = wave; u < pairs; u += 4) rows_layer<RB, 2>(L, 64 * u, a, b, Xin, pitch_in, Xout, pitch_out);
      if ((L.C & 32) && wave == (pairs & 3)) rows_layer<RB, 1>(L, 64 * pairs, a, b, Xin, pitch_in, Xout, pitch_out);
      off += 2 * L.C;
      __syncthreads();
    }
    for (int q = tid; q < TR * opr; q += 256) {
      const int row = q / opr, col = (q - row * opr) * 8;
      const long long p = p0 + row;
      if (p < g.n)
        *reinterpret_cast<uint4 *>(g.out + p * last.C + col) = *reinterpret_cast<const uint4 *>(Xlast + row * pitch_last + col);
    }
  }
}

// rows per tile, LDS pitches (e16 elements) and bytes of a shape; false: a shape the kernel does not take.  The tile has 64
// rows where that fits the CU's LDS and 32 where it does not (1024 -> 512 -> 512): the ONE rule, a function of the shape alone.
static bool rows_layout(int kpad, int nlayers, const int *widths, int *tr, int *pitch_a, int *pitch_b, int *sum_c,
                        long long *bytes) {
  if (nlayers < 1 || nlayers > kInferMaxLayers || !widths) return false;
  if (kpad < 32 || (kpad % 32) || kpad > kRowsInferMaxK) return false;
  int sum = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (widths[l] < 32 || (widths[l] % 32) || widths[l] > kInferMaxC) return false;
    sum += widths[l];
  }
  int wa = kpad, wb = widths[0];
  if (nlayers >= 2 && widths[1] > wa) wa = widths[1];
  if (nlayers == 3 && widths[2] > wb) wb = widths[2];
  const int pa = wa + kInferRowPad, pb = wb + kInferRowPad;
  int rows = 64;
  long long total = 8ll * sum + 2ll * rows * (pa + pb);
  if (total > kInferLdsLimit) {
    rows = 32;
    total = 8ll * sum + 2ll * rows * (pa + pb);
  }
  if (total > kInferLdsLimit) return false;
  *tr = rows;
  *pitch_a = pa;
  *pitch_b = pb;
  *sum_c = sum;
  *bytes = total;
  return true;
}

template <int RB>
static void rows_infer_launch(const RowsArgs &g, int grid, int lds, hipStream_t stream) {
  auto kern = rows_infer_kernel<RB>;
  static const hipError_t prepared = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, kInferLdsLimit);
  (void)prepared;
  kern<<<grid, 256, lds, stream>>>(g);
}

}  // namespace omnipq

using namespace omnipq;

extern "C" const char *omnipq_rows_infer_layer_record(void) {
  static_assert(sizeof(omnipq_rows_infer_layer) == 64 && sizeof(void *) == 8, "omnipq_rows_infer_layer: size");
  static_assert(offsetof(omnipq_rows_infer_layer, W) == 0, "omnipq_rows_infer_layer.W: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, ldw) == 8, "omnipq_rows_infer_layer.ldw: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, C) == 12, "omnipq_rows_infer_layer.C: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, bias) == 16, "omnipq_rows_infer_layer.bias: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, gamma) == 24, "omnipq_rows_infer_layer.gamma: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, beta) == 32, "omnipq_rows_infer_layer.beta: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, running_mean) == 40, "omnipq_rows_infer_layer.running_mean: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, running_var) == 48, "omnipq_rows_infer_layer.running_var: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, eps) == 56, "omnipq_rows_infer_layer.eps: offset");
  static_assert(offsetof(omnipq_rows_infer_layer, relu) == 60, "omnipq_rows_infer_layer.relu: offset");
  return "struct omnipq_rows_infer_layer W:p ldw:i C:i bias:p gamma:p beta:p running_mean:p running_var:p eps:f relu:i";
}

extern "C" long long omnipq_rows_infer_lds_bytes(int kpad, int nlayers, const int *widths) {
  int tr, pa, pb, sum;
  long long bytes;
  return rows_layout(kpad, nlayers, widths, &tr, &pa, &pb, &sum, &bytes) ? bytes : -1;
}

extern "C" int omnipq_rows_infer(long long n, int cin, long long ldx, const void *x, int x_is_f32, int nlayers,
                                 const void *layers, void *out16, void *stream) {
  if (n < 0 || cin <= 0 || cin > kRowsInferMaxK || ldx < cin) return OMNIPQ_EINVAL;
  if (nlayers < 1 || nlayers > kInferMaxLayers || !layers) return OMNIPQ_EINVAL;
  const omnipq_rows_infer_layer *rec = static_cast<const omnipq_rows_infer_layer *>(layers);
  const int kpad = (cin + 31) / 32 * 32;
  int widths[kInferMaxLayers];
  for (int l = 0; l < nlayers; ++l) widths[l] = rec[l].C;
  RowsArgs g;
  int tr;
  long long bytes;
  if (!rows_layout(kpad, nlayers, widths, &tr, &g.pitch_a, &g.pitch_b, &g.sum_c, &bytes)) return OMNIPQ_EINVAL;
  for (int l = 0; l < nlayers; ++l) {
    const int K = l == 0 ? kpad : widths[l - 1];
    const int bn = (rec[l].gamma != NULL) + (rec[l].beta != NULL) + (rec[l].running_mean != NULL) + (rec[l].running_var != NULL);
    if (!rec[l].W || (bn != 0 && bn != 4)) return OMNIPQ_EINVAL;
    if (rec[l].ldw < K || (rec[l].ldw % 8)) return OMNIPQ_EINVAL;
    g.lay[l] = RowsLayer{(const e16_t *)rec[l].W, rec[l].ldw, rec[l].C, K, (bn == 4 || rec[l].relu) ? 1 : 0, rec[l].bias,
                         rec[l].gamma, rec[l].beta, rec[l].running_mean, rec[l].running_var, rec[l].eps};
  }
  if (!x || !out16 || ((size_t)out16 % 16)) return OMNIPQ_EINVAL;
  const long long tiles = (n + tr - 1) / tr;
  if (tiles > 0x7fffffffll) return OMNIPQ_ETOOLARGE;
  if (n == 0) return OMNIPQ_OK;
  g.n = n;
  g.ldx = ldx;
  g.cin = cin;
  g.kpad = kpad;
  g.nlayers = nlayers;
  g.tiles = (int)tiles;
  g.x_f32 = x_is_f32 ? 1 : 0;
  // 16-byte loads of the input where every piece of a row is aligned
  g.x_vec = (!x_is_f32 && (ldx % 8) == 0 && ((size_t)x % 16) == 0) ? 1 : 0;
  g.x = x;
  g.out = (e16_t *)out16;
  // persistent workgroups: as many as stay resident (LDS; two waves per SIMD at the tile functions' ~200 registers)
  long long per_cu = kInferLdsLimit / bytes;
  if (per_cu > 2) per_cu = 2;
  long long grid = per_cu * infer_cus();
  if (grid > tiles) grid = tiles;
  if (tr == 64)
    rows_infer_launch<2>(g, (int)grid, (int)bytes, (hipStream_t)stream);
  else
    rows_infer_launch<1>(g, (int)grid, (int)bytes, (hipStream_t)stream);
  OMNIPQ_LAUNCH_CHECK();
  return OMNIPQ_OK;
}
