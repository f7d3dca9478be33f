// The oriented-box IoU of csrc/eval_iou.hip as functions of plain C++: what a thread of the two kernels computes.  Device code
// under hipcc; compiled as host C++ (no HIP, `lds` any array of kIouRows * kIouThreads doubles) it is the kernels' CPU twin, which
// tests/test_obb_iou_host_twin.py (tests/obb_iou_host_twin.cpp) holds against eval_det.box3d_iou under AddressSanitizer.
#pragma once
#include <math.h>

#ifdef __HIP__
#define OMNIPQ_HD __device__ __forceinline__
#define OMNIPQ_RESTRICT __restrict__
#else
#define OMNIPQ_HD inline
#define OMNIPQ_RESTRICT
#endif

namespace omnipq {

// How many vertices a clip can produce.  One pass of Sutherland-Hodgman over a polygon of n vertices emits every vertex
// that tests inside and one point per edge whose ends test differently.  With c such edges (c is even and c <= n) the
// vertices fall into c / 2 runs outside of at least one vertex each, so at most n - c / 2 are emitted, n + c / 2 <= n + n / 2
// points in all.  This counts test OUTCOMES only: it holds whatever the rounded arithmetic, infinities or NaNs make of the
// geometry (in exact arithmetic two convex quadrilaterals give 8).  From 4 vertices: 6, 9, 13 after the first three edges
// of the clip polygon.  The output of the fourth edge is not stored: its area is accumulated as the points are emitted.
// The two ping-pong buffers therefore hold 9 (inputs of 4 and 9: the subject, the second output) and 13 vertices (6 and 13).
constexpr int kIouThreads = 64;
constexpr int kIouBufA = 9, kIouBufB = 13;                      // vertices per thread
constexpr int kIouRows = 2 * (kIouBufA + kIouBufB);             // LDS rows of kIouThreads doubles: x and y per vertex

// The polygon whose area box3d_iou asks for, taken as its points are emitted: _shoelace's two sums
//   s1 = sum_i x[i] y[i-1]   s2 = sum_i y[i] x[i-1]   (np.roll(., 1): the predecessor, cyclic)
// with the term of the first point, which needs the last one, added at the end.
struct Shoelace {
  double s1 = 0.0, s2 = 0.0, x0 = 0.0, y0 = 0.0, xp = 0.0, yp = 0.0;
  int n = 0;
  OMNIPQ_HD void add(double x, double y) {
    if (n == 0) {
      x0 = x, y0 = y;
    } else {
      s1 = s1 + x * yp;
      s2 = s2 + y * xp;
    }
    xp = x, yp = y;
    ++n;
  }
  // 0.5 * abs(dot(x, roll(y, 1)) - dot(y, roll(x, 1))) if len(poly) >= 3 else 0.0
  OMNIPQ_HD double area() const {
    if (n < 3) return 0.0;
    const double a = s1 + x0 * yp, b = s2 + y0 * xp;
    return 0.5 * fabs(a - b);
  }
};

// One box as box3d_iou reads it: the footprint (x, z) of corners 3, 2, 1, 0, the two heights, _volume.
struct ObbBox {
  double fx[4], fy[4], top, bottom, area, volume;
};

OMNIPQ_HD double dist3(const double *OMNIPQ_RESTRICT p, const double *OMNIPQ_RESTRICT q) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);                   // numpy's sum over three elements runs left to right
}

OMNIPQ_HD ObbBox load_box(const double *OMNIPQ_RESTRICT c) {
  ObbBox b;
  Shoelace sh;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b.fx[i] = c[(3 - i) * 3];
    b.fy[i] = c[(3 - i) * 3 + 2];
    sh.add(b.fx[i], b.fy[i]);
  }
  b.area = sh.area();
  b.top = c[1];                                                 // c[0, 1]
  b.bottom = c[4 * 3 + 1];                                      // c[4, 1]
  b.volume = dist3(c, c + 3) * dist3(c + 3, c + 6) * dist3(c, c + 12);
  return b;
}

// box3d_iou(corners1 = p, corners2 = g) -> iou3d, iou2d.  `lds` is the calling thread's slice: row r at lds[r * kIouThreads].
OMNIPQ_HD void obb_iou(const ObbBox &p, const ObbBox &g, double *OMNIPQ_RESTRICT lds, double &iou3d,
                                        double &iou2d) {
  // _clip(rect1, rect2): the subject is p's footprint, the clip polygon g's
  double *src = lds, *dst = lds + 2 * kIouBufA * kIouThreads;   // buffer A (9 vertices), buffer B (13)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    src[(2 * i) * kIouThreads] = p.fx[i];
    src[(2 * i + 1) * kIouThreads] = p.fy[i];
  }
  int n = 4;
  Shoelace inter;
  double ax = g.fx[3], ay = g.fy[3];                            // a = clip[-1]
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double bx = g.fx[k], by = g.fy[k];
    const bool last = k == 3;
    int m = 0;
    if (n > 0) {                                                // `if not out: return []`
      const double ex = bx - ax, ey = by - ay;
      double sx = src[(2 * (n - 1)) * kIouThreads], sy = src[(2 * (n - 1) + 1) * kIouThreads];     // s = src[-1]
      bool s_in = ex * (sy - ay) > ey * (sx - ax);
      for (int i = 0; i < n; ++i) {
        const double px = src[(2 * i) * kIouThreads], py = src[(2 * i + 1) * kIouThreads];
        const bool e_in = ex * (py - ay) > ey * (px - ax);
        if (e_in != s_in) {
          const double dcx = ax - bx, dcy = ay - by;
          const double dpx = sx - px, dpy = sy - py;
          const double n1 = ax * by - ay * bx;
          const double n2 = sx * py - sy * px;
          const double n3 = 1.0 / (dcx * dpy - dcy * dpx);
          const double qx = (n1 * dpx - n2 * dcx) * n3, qy = (n1 * dpy - n2 * dcy) * n3;
          if (last) {
            inter.add(qx, qy);
          } else {
            dst[(2 * m) * kIouThreads] = qx;
            dst[(2 * m + 1) * kIouThreads] = qy;
          }
          ++m;
        }
        if (e_in) {
          if (last) {
            inter.add(px, py);
          } else {
            dst[(2 * m) * kIouThreads] = px;
            dst[(2 * m + 1) * kIouThreads] = py;
          }
          ++m;
        }
        sx = px, sy = py, s_in = e_in;
      }
    }
    n = m;
    double *t = src;
    src = dst, dst = t;
    ax = bx, ay = by;
  }
  const double inter_area = inter.area();
  iou2d = inter_area / (p.area + g.area - inter_area);
  const double ymax = g.top < p.top ? g.top : p.top;            // min(c1[0, 1], c2[0, 1]) as Python's min decides
  const double ymin = g.bottom > p.bottom ? g.bottom : p.bottom;
  const double dh = ymax - ymin;
  const double inter_vol = inter_area * (dh > 0.0 ? dh : 0.0);  // max(0.0, ymax - ymin)
  iou3d = inter_vol / (p.volume + g.volume - inter_vol);
}

}  // namespace omnipq
