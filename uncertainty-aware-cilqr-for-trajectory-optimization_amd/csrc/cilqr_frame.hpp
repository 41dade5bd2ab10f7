// cilqr_frame.hpp — the arithmetic of the path-aligned planning frame, written once for the framed pre-step (local_plan.hip) and
// the transforms (cilqr_frame.hip).  include/cilqr.h states the order of every operation; the tests restate it in numpy and
// compare bits, so nothing here may be contracted into a fused multiply-add or reassociated.
#pragma once

#include <hip/hip_runtime.h>

#include "cilqr.h"

namespace cilqr {
namespace frame {

struct Frame {
  double ox, oy, c, s, phi;
};

__device__ __forceinline__ Frame load_frame(const double* f) {
  Frame r;
  r.ox = f[0]; r.oy = f[1]; r.c = f[2]; r.s = f[3]; r.phi = f[4];
  return r;
}

// Origin o, chord end e and slice length n → the frame and its CILQR_FRAME_DEGENERATE bit.
__device__ __forceinline__ Frame make_frame(double ox, double oy, double ex, double ey, int n, int* info) {
#pragma clang fp contract(off)
  const double dx = ex - ox, dy = ey - oy;
  const double h = sqrt(dx * dx + dy * dy);
  Frame r;
  r.ox = ox; r.oy = oy;
  if (n < 2 || h == 0.0 || !(fabs(h) <= 1.7976931348623157e308)) {
    r.c = 1.0; r.s = 0.0; r.phi = 0.0;
    *info |= CILQR_FRAME_DEGENERATE;
  } else {
    r.c = dx / h;
    r.s = dy / h;
    r.phi = atan2(r.s, r.c);
  }
  return r;
}

// x' = c·(x − ox) + s·(y − oy), y' = c·(y − oy) − s·(x − ox): every product and the one sum rounded on its own.
__device__ __forceinline__ void point_to(const Frame& f, double x, double y, double* xf, double* yf) {
#pragma clang fp contract(off)
  const double ux = x - f.ox, uy = y - f.oy;
  const double a = f.c * ux, b = f.s * uy, c = f.c * uy, d = f.s * ux;
  *xf = a + b;
  *yf = c - d;
}

// x = (c·x' − s·y') + ox, y = (s·x' + c·y') + oy.
__device__ __forceinline__ void point_from(const Frame& f, double xf, double yf, double* x, double* y) {
#pragma clang fp contract(off)
  const double a = f.c * xf, b = f.s * yf, c = f.s * xf, d = f.c * yf;
  const double rx = a - b, ry = c + d;
  *x = rx + f.ox;
  *y = ry + f.oy;
}

}  // namespace frame
}  // namespace cilqr
