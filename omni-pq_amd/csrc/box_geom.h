// Corners and extents of one oriented box, shared by csrc/eval_ops.hip (box_corners_kernel) and csrc/detect.hip
// (decode_boxes_kernel) so that the two produce the same bits: utils/box_util.py:218-233 `get_3d_box` after
// flip_axis_to_camera, f64 arithmetic on the f32 cosine / sine of an f32 heading.  Compile every user with -ffp-contract=off.
#pragma once
#include "common.h"

namespace omnipq {

// centre (cx, cy, cz) f32 in the depth frame, size (l, w, h) f64, heading f32 -> corners8 [8][3] and aabb [6]
// (x1, y1, z1, x2, y2, z2) in the upright-camera frame; either output may be NULL
__device__ __forceinline__ void box_corners_of(float ang, double l, double w, double h, float cx, float cy, float cz,
                                               double *__restrict__ corners8, double *__restrict__ aabb) {
  const double c = (double)cosf(ang), s = (double)sinf(ang);
  const double ccx = (double)cx, ccy = (double)(-cz), ccz = (double)cy;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double x = ((i & 3) < 2 ? l : -l) / 2;
    const double y = (i < 4 ? h : -h) / 2;
    const double z = ((i & 3) == 0 || (i & 3) == 3 ? w : -w) / 2;
    const double p[3] = {c * x + s * z + ccx, y + ccy, -s * x + c * z + ccz};
    for (int a = 0; a < 3; ++a) {
      if (corners8) corners8[i * 3 + a] = p[a];
      lo[a] = fmin(lo[a], p[a]);
      hi[a] = fmax(hi[a], p[a]);
    }
  }
  if (aabb)
    for (int a = 0; a < 3; ++a) {
      aabb[a] = lo[a];
      aabb[3 + a] = hi[a];
    }
}

}  // namespace omnipq
