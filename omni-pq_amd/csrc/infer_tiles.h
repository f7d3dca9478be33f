// Tile functions of the inference chains (csrc/sa_infer.hip: a set-abstraction stage; csrc/rows_infer.hip: a per-point stack;
// DESIGN.md 4.8, 4.9): a workgroup of four waves keeps a tile of rows in LDS and takes it through a stack of linear layers whose
// BatchNorm is a known affine.  A wave owns 64 (or a last 32) output channels for ALL rows of the tile; W fragments come from
// global memory / L2 (every weight is read once per workgroup and tile), X fragments from LDS.  Rows in LDS carry kInferRowPad
// elements (16 bytes) behind them, which keeps the 16-byte fragment reads of 32 consecutive rows off each other's banks.
#pragma once
#include "common.h"

namespace omnipq {

constexpr int kInferMaxLayers = 3;
constexpr int kInferMaxC = 640;
constexpr int kInferLdsLimit = 160 * 1024;       // LDS of one CU
constexpr int kInferRowPad = 8;                  // e16 elements behind every LDS row
constexpr int kInferPrefetch = 4;                // 32-wide K units of W fragments in flight per wave

__device__ __forceinline__ e16x8 infer_load8(const e16_t *p) { return *reinterpret_cast<const e16x8 *>(p); }

// acc[j][rb] (+)= over K of the 32 x 32 blocks (weight rows c0 + 32 j .., tile rows 32 rb ..).  TRANSPOSED: the weight block is
// the A operand (accumulator: lane = tile row, registers = channels), else the B operand (lane = channel, registers = rows).
template <int RB, int NCB, bool TRANSPOSED>
__device__ __forceinline__ void infer_block_gemm(const e16_t *__restrict__ W, int ldw, int K, int c0, const e16_t *X, int pitch,
                                                 omnipq_f32x16 (&acc)[NCB][RB]) {
  const int lane = lane_id(), r = lane & 31, h = lane >> 5;
  const e16_t *wrow[NCB];
#pragma unroll
  for (int j = 0; j < NCB; ++j) {
    wrow[j] = W + (size_t)(c0 + 32 * j + r) * ldw + 8 * h;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[j][rb][i] = 0.f;
  }
  const e16_t *xrow = X + r * pitch + 8 * h;
  const int units = K >> 5;
  e16x8 w[kInferPrefetch][NCB][2];
#pragma unroll
  for (int u = 0; u < kInferPrefetch; ++u)
    if (u < units) {
#pragma unroll
      for (int j = 0; j < NCB; ++j) {
        w[u][j][0] = infer_load8(wrow[j] + 32 * u);
        w[u][j][1] = infer_load8(wrow[j] + 32 * u + 16);
      }
    }
  for (int u0 = 0; u0 < units; u0 += kInferPrefetch) {
#pragma unroll
    for (int q = 0; q < kInferPrefetch; ++q) {
      const int u = u0 + q;
      if (u < units) {                       // wave-uniform
        e16x8 w0[NCB], w1[NCB];
#pragma unroll
        for (int j = 0; j < NCB; ++j) {
          w0[j] = w[q][j][0];
          w1[j] = w[q][j][1];
        }
        if (u + kInferPrefetch < units) {
#pragma unroll
          for (int j = 0; j < NCB; ++j) {
            w[q][j][0] = infer_load8(wrow[j] + 32 * (u + kInferPrefetch));
            w[q][j][1] = infer_load8(wrow[j] + 32 * (u + kInferPrefetch) + 16);
          }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const e16x8 x0 = infer_load8(xrow + 32 * rb * pitch + 32 * u);
          const e16x8 x1 = infer_load8(xrow + 32 * rb * pitch + 32 * u + 16);
#pragma unroll
          for (int j = 0; j < NCB; ++j) {
            if (TRANSPOSED) {
              acc[j][rb] = mfma_e16_32x32x16(w0[j], x0, acc[j][rb]);
              acc[j][rb] = mfma_e16_32x32x16(w1[j], x1, acc[j][rb]);
            } else {
              acc[j][rb] = mfma_e16_32x32x16(x0, w0[j], acc[j][rb]);
              acc[j][rb] = mfma_e16_32x32x16(x1, w1[j], acc[j][rb]);
            }
          }
        }
      }
    }
  }
}

// a layer's channels [c0, c0 + 32 NCB) into LDS: Xout[row][c] = e16(relu(a[c] acc + b[c])), one rounding (RELU false: no relu)
template <int RB, int NCB, bool RELU = true>
__device__ __forceinline__ void infer_hidden(const e16_t *__restrict__ W, int ldw, int K, int c0, const float *a, const float *b,
                                             const e16_t *Xin, int pitch_in, e16_t *Xout, int pitch_out) {
  omnipq_f32x16 acc[NCB][RB];
  infer_block_gemm<RB, NCB, true>(W, ldw, K, c0, Xin, pitch_in, acc);
  const int lane = lane_id(), r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < NCB; ++j)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int c = c0 + 32 * j + 8 * g4 + 4 * h;          // registers 4 g4 .. 4 g4 + 3: channels c .. c + 3
      const float4 a4 = *reinterpret_cast<const float4 *>(a + c);
      const float4 b4 = *reinterpret_cast<const float4 *>(b + c);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        float v0 = a4.x * acc[j][rb][4 * g4 + 0] + b4.x;
        float v1 = a4.y * acc[j][rb][4 * g4 + 1] + b4.y;
        float v2 = a4.z * acc[j][rb][4 * g4 + 2] + b4.z;
        float v3 = a4.w * acc[j][rb][4 * g4 + 3] + b4.w;
        if (RELU) {
          v0 = fmaxf(v0, 0.f);
          v1 = fmaxf(v1, 0.f);
          v2 = fmaxf(v2, 0.f);
          v3 = fmaxf(v3, 0.f);
        }
        uint2 o;
        o.x = pack_e16x2(v0, v1);
        o.y = pack_e16x2(v2, v3);
        *reinterpret_cast<uint2 *>(Xout + (32 * rb + r) * pitch_out + c) = o;
      }
    }
}

// compute units of the current device (persistent grids are sized by it); 256 where it cannot be asked
static inline int infer_cus() {
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}

}  // namespace omnipq
