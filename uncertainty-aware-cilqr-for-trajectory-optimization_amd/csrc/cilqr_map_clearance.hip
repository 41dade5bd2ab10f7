// cilqr_map_clearance.hip — exact clearance of the vehicle's rectangle to the occupied cells of the map set on the handle
// (cilqr_map_clearance*, include/cilqr.h): the map counterpart of CILQR_FP_CLEARANCE.  Where cilqr_footprint_check says whether the
// rectangle covers an occupied cell, this says how far the nearest occupied cell centre is, and how deep the deepest one lies.
//
// Nothing here is a floating-point sum: (min clearance, lowest cell) and (min clearance, lowest step) are lexicographic and the rest
// are integer counts, so a row's bits depend on that row's inputs alone and the mapping is free:
//   steps  wavefront = (row, step), four steps per workgroup, rows·ceil(N/4) workgroups (the footprint map kernel's mapping).  The
//          rectangle's centre and heading in the map frame are wavefront-uniform and moved to scalar registers; the WINDOW of
//          virtual cell indices comes from footprint_range (cilqr_footprint_range.h: formed in doubles, compared with ±2^30 before
//          any conversion) called with the half-extents grown by `reach`.  Lanes stride over i, so a wavefront reads consecutive
//          floats of the column-major layer; the loop runs over the window clipped to the map and every load is guarded by the in-map
//          test of its own (i, j).  A seed's signed clearance s enters the minimum only where s <= reach: the window's shape
//          decides nothing.
//   fold   one wavefront per row folds the N step records into mc and total.
// No global atomics, no LDS, no scratch memory.
#include "cilqr_footprint_range.h"
#include "cilqr_map_probes.hpp"

namespace cilqr {

using namespace dev;

namespace {

// (min value, lowest index); a NaN never wins
__device__ __forceinline__ void cmin_merge(double& c0, int& e0, double c1, int e1) {
  if (c1 < c0 || (c1 == c0 && e1 < e0)) { c0 = c1; e0 = e1; }
}

__global__ __launch_bounds__(FOOTPRINT_THREADS) void cilqr_map_clearance_steps_kernel(MapClearanceArgs a) {
#pragma clang fp contract(off)  // cell centres as the footprint check forms them; the definition's formulas as C evaluates them
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int N = a.s.N, G = (N + FOOTPRINT_WAVES - 1) / FOOTPRINT_WAVES;
  const int row = blockIdx.x / G, t = (blockIdx.x - row * G) * FOOTPRINT_WAVES + wave;  // (wavefront-uniform)
  if (t >= N) return;  // (a workgroup's last wavefronts idle where N is no multiple of four; the kernel has no barrier)
  const int b = row / a.S;
  const double* X = a.X + ((size_t)row * ((size_t)N + 1) + t) * 4;
  const double x = X[0], y = X[1], th = X[3];
  bool lost = !(is_finite(x) && is_finite(y) && is_finite(th));
  FootprintRange r = {0, -1, 0, -1, 0};
  double cx = 0.0, cy = 0.0, cm = 1.0, sm = 0.0;
  if (!lost) {
    double st, ct;
    sincos_fast(th, &st, &ct);
    const UncPose po = unc_pose(a.s.unc, b);
    double qx[4], qy[4];
    footprint_corners(x, y, ct, st, a.hl + a.reach, a.hw + a.reach, po.px, po.py, po.cp, po.sp, qx, qy);
#pragma unroll
    for (int k = 0; k < 4; ++k) { qx[k] = uniform_double(qx[k]); qy[k] = uniform_double(qy[k]); }
    r = footprint_range(qx, qy, a.s.unc.x_first, a.s.unc.y_first, a.s.unc.inv_res);
    lost = !r.ok;  // (a window whose index range leaves ±2^30 is lost as a state that is not finite is)
    // the rectangle's centre and heading in the map frame: the rigid transform of the corners
    const double dx = x - po.px, dy = y - po.py;
    cx = uniform_double(po.cp * dx + po.sp * dy);
    cy = uniform_double(po.cp * dy - po.sp * dx);
    cm = uniform_double(ct * po.cp + st * po.sp);
    sm = uniform_double(st * po.cp - ct * po.sp);
  }

  double best = __builtin_huge_val();
  int best_c = NO_INDEX;
  bool leaves = false;
  if (!lost) {
    const int rows = a.s.unc.rows, cols = a.s.unc.cols;
    leaves = r.i_lo < 0 || r.j_lo < 0 || r.i_hi > rows - 1 || r.j_hi > cols - 1;
    const LayerPtr layer = (LayerPtr)(a.s.unc.layer + (size_t)b * (size_t)a.s.unc.stride);
    const double x_first = a.s.unc.x_first, y_first = a.s.unc.y_first, res = a.res, threshold = a.occ_threshold;
    const double hl = a.hl, hw = a.hw, reach = a.reach;
    const bool nan_seeds = (a.flags & CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS) != 0;
    const int i_lo = max(r.i_lo, 0), i_hi = min(r.i_hi, rows - 1), j_lo = max(r.j_lo, 0), j_hi = min(r.j_hi, cols - 1);
    for (int j = j_lo; j <= j_hi; ++j) {  // (uniform)
      const double py = y_first + res * (double)(-j);
      const double db = py - cy;
      for (int i0 = i_lo; i0 <= i_hi; i0 += WAVE) {
        const int i = i0 + lane;
        // (the only load of the layer: of a cell inside [0, rows) x [0, cols))
        if (i <= i_hi && i >= 0 && i < rows && j >= 0 && j < cols) {
          const float v = layer[(size_t)j * rows + i];
          const bool seed = v == v ? (fabsf(v) <= 3.4028234663852886e38f && (double)v > threshold) : nan_seeds;
          if (seed) {
            const double px = x_first + res * (double)(-i);
            const double da = px - cx;
            const double ba = da * cm + db * sm, bb = db * cm - da * sm;
            const double ua = fabs(ba) - hl, ub = fabs(bb) - hw;
            double s;
            if (ua > 0.0 || ub > 0.0) {
              const double u = fmax(ua, 0.0), w = fmax(ub, 0.0);
              s = sqrt(u * u + w * w);
            } else {
              s = fmax(ua, ub);  // minus the penetration depth, 0 on the boundary
            }
            if (s <= reach) cmin_merge(best, best_c, s, i + j * rows);
          }
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) cmin_merge(best, best_c, __shfl_xor(best, o, WAVE), __shfl_xor(best_c, o, WAVE));
  if (lane == 0) {
    const size_t at = (size_t)row * N + t;
    a.step_clearance[at] = lost ? -__builtin_huge_val() : best;
    double* rec = a.steps + at * MAP_CLEARANCE_STEP_REC;
    rec[0] = best_c == NO_INDEX ? -1.0 : (double)best_c;
    rec[1] = (double)((leaves ? 1 : 0) | (lost ? 2 : 0));
  }
}

// One wavefront per row: the N step records → mc [CILQR_MAP_CLEARANCE_FIELDS] and total.
__global__ __launch_bounds__(WAVE) void cilqr_map_clearance_fold_kernel(MapClearanceArgs a) {
  const int row = blockIdx.x, lane = threadIdx.x, N = a.s.N;
  const double* clr = a.step_clearance + (size_t)row * N;
  const double* rec = a.steps + (size_t)row * N * MAP_CLEARANCE_STEP_REC;
  double best = __builtin_huge_val();
  int best_t = NO_INDEX, below = 0, first = NO_INDEX, touch = 0, off = 0, lost = 0;
  for (int t = lane; t < N; t += WAVE) {
    const double c = clr[t];
    const int fl = (int)rec[(size_t)t * MAP_CLEARANCE_STEP_REC + 1];
    if (c < __builtin_huge_val()) cmin_merge(best, best_t, c, t);
    if (c < a.min_clearance) { ++below; first = min(first, t); }
    if (c <= 0.0) ++touch;
    if (fl & 1) ++off;
    if (fl & 2) ++lost;
  }
  for (int o = 32; o > 0; o >>= 1) {
    cmin_merge(best, best_t, __shfl_xor(best, o, WAVE), __shfl_xor(best_t, o, WAVE));
    below += __shfl_xor(below, o, WAVE);
    first = min(first, __shfl_xor(first, o, WAVE));
    touch += __shfl_xor(touch, o, WAVE);
    off += __shfl_xor(off, o, WAVE);
    lost += __shfl_xor(lost, o, WAVE);
  }
  if (lane == 0) {
    double* out = a.mc + (size_t)row * CILQR_MAP_CLEARANCE_FIELDS;
    out[CILQR_MC_CLEARANCE] = best;
    out[CILQR_MC_STEP] = best_t == NO_INDEX ? -1.0 : (double)best_t;
    out[CILQR_MC_CELL] = best_t == NO_INDEX ? -1.0 : rec[(size_t)best_t * MAP_CLEARANCE_STEP_REC];
    out[CILQR_MC_BELOW_STEPS] = (double)below;
    out[CILQR_MC_FIRST_BELOW] = first == NO_INDEX ? -1.0 : (double)first;
    out[CILQR_MC_TOUCH_STEPS] = (double)touch;
    out[CILQR_MC_OFF_MAP_STEPS] = (double)off;
    out[CILQR_MC_LOST_STEPS] = (double)lost;
    if (a.total) {
      const double base = a.base[row];
      a.total[row] = is_finite(base) && lost == 0 && best >= a.min_clearance ? base : __builtin_nan("");
    }
  }
}

}  // namespace

hipError_t launch_map_clearance(const MapClearanceArgs& a, hipStream_t stream) {
  if (a.rows <= 0 || a.s.N <= 0) return hipSuccess;
  const long long blocks = (long long)a.rows * ((a.s.N + FOOTPRINT_WAVES - 1) / FOOTPRINT_WAVES);
  hipLaunchKernelGGL(cilqr_map_clearance_steps_kernel, dim3((unsigned)blocks), dim3(FOOTPRINT_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_map_clearance_fold_kernel, dim3(a.rows), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
