// cilqr_footprint_range.h — the ego rectangle of cilqr_footprint_check in the map frame and the range of VIRTUAL cell indices
// its cells can lie in: plain C++ that the kernel (cilqr_footprint.hip) and a CPU program (tests/cpp/footprint_range_dump.cpp)
// compile alike, so that the only place where a double becomes an index is exercised without a GPU — with states a million
// metres away, at 1e300, infinite and NaN.
//
// Virtual grid: cell (i, j) has its centre at (x_first - i·res, y_first - j·res) for EVERY integer i, j, the formula of the
// map's own cells (G/grid_map_core/src/GridMapMath.cpp:114-127) continued beyond [0, rows) x [0, cols).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define CILQR_FP_HD __host__ __device__ inline
#else
#define CILQR_FP_HD inline
#endif

namespace cilqr {

constexpr double FOOTPRINT_INDEX_LIMIT = 1073741824.0;  // 2^30: every index a range names, and every sum of two, fits an int32

// The four corners in bondingBoxHandle's order (hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw) (M/src/local_costmap.cpp:860-922) of
// the rectangle centred on (x, y) with heading cosine / sine (ct, st), taken into the map frame whose pose in the planning frame is
// (px, py) with heading cosine / sine (cp, sp): the rigid transform of the map cost's probes (unc_cost_add).
CILQR_FP_HD void footprint_corner(double a, double b, double x, double y, double ct, double st, double px, double py, double cp, double sp,
                                  double& qx, double& qy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double Px = x + (a * ct - b * st), Py = y + (a * st + b * ct);
  const double dx = Px - px, dy = Py - py;
  qx = cp * dx + sp * dy;
  qy = cp * dy - sp * dx;
}
CILQR_FP_HD void footprint_corners(double x, double y, double ct, double st, double hl, double hw, double px, double py, double cp,
                                   double sp, double (&qx)[4], double (&qy)[4]) {
  footprint_corner(hl, hw, x, y, ct, st, px, py, cp, sp, qx[0], qy[0]);
  footprint_corner(hl, -hw, x, y, ct, st, px, py, cp, sp, qx[1], qy[1]);
  footprint_corner(-hl, -hw, x, y, ct, st, px, py, cp, sp, qx[2], qy[2]);
  footprint_corner(-hl, hw, x, y, ct, st, px, py, cp, sp, qx[3], qy[3]);
}

struct FootprintRange {
  int i_lo, i_hi, j_lo, j_hi;  // inclusive; empty (lo = 0, hi = -1) when !ok
  int ok;                      // 0: a corner is not finite, or an index of the range lies beyond ±2^30
};

// Every virtual cell whose centre can pass Polygon::isInside for the corners lies in the returned range: a centre inside the
// 4-gon lies within the corners' extremes, which are widened by one cell on every side against the rounding of the division
// (at most 2^30·2^-52 of a cell).  The range is formed in doubles and compared with ±2^30 BEFORE any conversion to int.
CILQR_FP_HD FootprintRange footprint_range(const double (&qx)[4], const double (&qy)[4], double x_first, double y_first, double inv_res) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FootprintRange r = {0, -1, 0, -1, 0};
  bool finite = true;
  double x_min = qx[0], x_max = qx[0], y_min = qy[0], y_max = qy[0];
  for (int k = 0; k < 4; ++k) {
    finite = finite && fabs(qx[k]) < 1.7e308 && fabs(qy[k]) < 1.7e308;  // (NaN fails the comparison)
    x_min = qx[k] < x_min ? qx[k] : x_min; x_max = qx[k] > x_max ? qx[k] : x_max;
    y_min = qy[k] < y_min ? qy[k] : y_min; y_max = qy[k] > y_max ? qy[k] : y_max;
  }
  if (!finite) return r;
  // i grows as x falls: the largest x gives the lowest index
  const double i_lo = floor((x_first - x_max) * inv_res) - 1.0, i_hi = ceil((x_first - x_min) * inv_res) + 1.0;
  const double j_lo = floor((y_first - y_max) * inv_res) - 1.0, j_hi = ceil((y_first - y_min) * inv_res) + 1.0;
  const double L = FOOTPRINT_INDEX_LIMIT;
  if (!(i_lo >= -L && i_hi <= L && j_lo >= -L && j_hi <= L && i_lo <= i_hi && j_lo <= j_hi)) return r;  // (NaN and inf fail)
  r.i_lo = (int)i_lo; r.i_hi = (int)i_hi; r.j_lo = (int)j_lo; r.j_hi = (int)j_hi;
  r.ok = 1;
  return r;
}

}  // namespace cilqr
