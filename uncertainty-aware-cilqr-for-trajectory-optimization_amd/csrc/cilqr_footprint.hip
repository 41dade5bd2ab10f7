// cilqr_footprint.hip — the exact footprint check (cilqr_footprint_check*, include/cilqr.h): the vehicle's rectangle, not the
// solver's surrogates, against the obstacles' rectangles (a separating-axis test and, where separated, the exact distance) and
// against the cells of the map set on the handle (Polygon::isInside of every cell centre under the rectangle: the cells
// cilqr_rasterize_polygons marks for the same vertices).  Geometry only: no speed inflation, no s_safe, no probes.
//
// Nothing here is a floating-point sum.  Counts are integers; (min clearance, lowest entry) and (max occupancy, lowest step, lowest
// cell) are lexicographic; a step's smallest clearance is a minimum of order-preserving 64-bit keys.  All of it comes out the same
// in any evaluation order, so a row's bits depend on that row's inputs alone, and the mapping is free:
//   boxes  one workgroup of 256 lanes per row.  The N ego records (x, y, cos, sin) are formed once in LDS; lanes stride over the
//          entries e = m·N + t: the obstacle's sincos, four gaps, and the eight point-to-rectangle distances only where the gaps
//          say separated.  Per lane (min, lowest entry), joined by butterflies and across the four wavefronts in LDS; per step an
//          LDS atomic minimum of the clearance's key and a hit flag every hitting lane stores 1 into.
//   map    wavefront = (row, step), four steps per workgroup, rows·ceil(N/4) workgroups.  The four corners in the map frame are
//          wavefront-uniform and moved to scalar registers; the range of VIRTUAL cell indices the footprint can cover comes from
//          footprint_range (cilqr_footprint_range.h: formed in doubles, compared with ±2^30 before any conversion, exercised on the
//          CPU).  An edge's crossing abscissa is formed once per column, as in polygon_is_inside (costmap_polygons.hpp): lane c
//          forms those of column c of a chunk of 64, and the columns are then walked uniformly, four at a time, with the
//          abscissae read out of that lane into scalar registers and the four columns' loads in flight together.  Lanes stride
//          over i, so a wavefront reads consecutive floats of the column-major layer.  Every load is guarded by the in-map test
//          of its own (i, j).
//   merge  one wavefront per row folds the N step records and the boxes' record into fp, step_occ and total.
// No global atomics.  No scratch memory, no spilled register, 128 vector registers at most (make check).
#include "cilqr_footprint_range.h"
#include "cilqr_map_probes.hpp"

namespace cilqr {

using namespace dev;

namespace {

// A double as an unsigned key of the same order (-0 below +0; no NaN arrives), and back.
__device__ __forceinline__ unsigned long long key_of(double v) {
  const unsigned long long w = __builtin_bit_cast(unsigned long long, v);
  return (w >> 63) ? ~w : (w | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// (min value, lowest entry); a NaN never wins
__device__ __forceinline__ void cmin_merge(double& c0, int& e0, double c1, int e1) {
  if (c1 < c0 || (c1 == c0 && e1 < e0)) { c0 = c1; e0 = e1; }
}

// Distance from the point (a, b) of a rectangle's body frame to that rectangle (half-extents hl, hw); 0 inside.
__device__ __forceinline__ double point_box(double a, double b, double hl, double hw) {
  const double u = fmax(fabs(a) - hl, 0.0), v = fmax(fabs(b) - hw, 0.0);
  return sqrt(u * u + v * v);
}

// Signed clearance of the ego rectangle (centre (ex, ey), heading cosine / sine (ec, es), half-extents (hl, hw)) and the obstacle
// rectangle (centre (ox, oy), heading oth, half-extents (ol, ow)): include/cilqr.h, "signed clearance of an entry".
__device__ __forceinline__ double box_clearance(double ex, double ey, double ec, double es, double hl, double hw, double ox, double oy,
                                                double oth, double ol, double ow) {
  double so, co;
  sincos_fast(oth, &so, &co);
  const double dx = ox - ex, dy = oy - ey;
  // a_E·a_O = b_E·b_O = cc;  a_E·b_O = ss;  b_E·a_O = -ss
  const double cc = ec * co + es * so, ss = es * co - ec * so;
  const double acc = fabs(cc), ass = fabs(ss);
  // the centres' difference in the ego's body frame and in the obstacle's
  const double dEa = dx * ec + dy * es, dEb = dy * ec - dx * es;
  const double dOa = dx * co + dy * so, dOb = dy * co - dx * so;
  const double g0 = fabs(dEa) - (hl + (ol * acc + ow * ass));
  const double g1 = fabs(dEb) - (hw + (ol * ass + ow * acc));
  const double g2 = fabs(dOa) - (ol + (hl * acc + hw * ass));
  const double g3 = fabs(dOb) - (ow + (hl * ass + hw * acc));
  const double g = fmax(fmax(g0, g1), fmax(g2, g3));
  if (!(g > 0.0)) return g;  // overlapping or touching: minus the least overlap (a NaN from values beyond the range returns as it is)
  double best = __builtin_huge_val();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double sa = (k & 1) ? -1.0 : 1.0, sb = (k & 2) ? -1.0 : 1.0;
    // the ego's vertex in the obstacle's frame; the obstacle's vertex in the ego's
    best = fmin(best, point_box(sa * hl * cc - sb * hw * ss - dOa, sa * hl * ss + sb * hw * cc - dOb, ol, ow));
    best = fmin(best, point_box(dEa + sa * ol * cc + sb * ow * ss, dEb - sa * ol * ss + sb * ow * cc, hl, hw));
  }
  return best;
}

// LDS (dynamic): [ego records: 4·N (x, y, cos, sin; cos NaN: the state is not finite)][step keys: N][clearance per wavefront: 4]
// | int32: [hit flag per step: N][entry per wavefront: 4]
__global__ __launch_bounds__(FOOTPRINT_THREADS) void cilqr_footprint_boxes_kernel(FootprintArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int N = a.s.N, M = a.s.M;
  const int row = blockIdx.x, b = row / a.S;
  double* ego = lds;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ego + 4 * (size_t)N);
  double* red_c = reinterpret_cast<double*>(keys + N);
  int* hit = reinterpret_cast<int*>(red_c + FOOTPRINT_WAVES);
  int* red_e = hit + N;
  const double* X = a.X + (size_t)row * 4 * ((size_t)N + 1);
  for (int t = tid; t < N; t += FOOTPRINT_THREADS) {
    const double x = X[4 * t], y = X[4 * t + 1], th = X[4 * t + 3];
    const bool ok = is_finite(x) && is_finite(y) && is_finite(th);
    double s = 0.0, c = __builtin_nan("");
    if (ok) sincos_fast(th, &s, &c);
    ego[4 * t] = x; ego[4 * t + 1] = y; ego[4 * t + 2] = c; ego[4 * t + 3] = s;
    keys[t] = key_of(__builtin_huge_val());
    hit[t] = ok ? 0 : 1;  // (a state that is not finite is a hit, whatever M is)
  }
  __syncthreads();

  double best = __builtin_huge_val();
  int best_e = NO_INDEX;
  const int E = M * N;  // (the host checked M·N < 2^31)
  for (int e = tid; e < E; e += FOOTPRINT_THREADS) {
    const int m = e / N, t = e - m * N;
    const double ex = ego[4 * t], ey = ego[4 * t + 1], ec = ego[4 * t + 2], es = ego[4 * t + 3];
    if (!(ec == ec)) continue;
    const long long at = (long long)b * a.s.obs_bs + (long long)m * a.s.obs_ms + (long long)t * a.s.obs_ts;
    const double* P = a.s.obs_pose + 4 * at;
    const double* D = a.s.obs_dim + 2 * at;
    const double ox = P[0], oy = P[1], oth = P[3], ol = 0.5 * D[0], ow = 0.5 * D[1];
    double clr = __builtin_nan("");
    if (is_finite(ox) && is_finite(oy) && is_finite(oth) && ol >= 0.0 && ow >= 0.0 && is_finite(ol) && is_finite(ow))
      clr = box_clearance(ex, ey, ec, es, a.hl, a.hw, ox, oy, oth, ol, ow);
    if (clr == clr) {
      cmin_merge(best, best_e, clr, e);
      atomicMin(&keys[t], key_of(clr));
    }
    if (!(clr > 0.0)) hit[t] = 1;  // touching collides; an entry without a clearance value is a hit
  }
  for (int o = 32; o > 0; o >>= 1) cmin_merge(best, best_e, __shfl_xor(best, o, WAVE), __shfl_xor(best_e, o, WAVE));
  if (lane == 0) { red_c[wave] = best; red_e[wave] = best_e; }
  __syncthreads();  // (every key and flag is final)
  for (int t = tid; t < N; t += FOOTPRINT_THREADS) {
    const size_t at = (size_t)row * N + t;
    const double c = ego[4 * t + 2];
    a.step_clearance[at] = c == c ? key_value(keys[t]) : -__builtin_huge_val();
    a.steps[at * FOOTPRINT_STEP_REC] = (double)hit[t];
  }
  if (tid == 0) {
    for (int v = 1; v < FOOTPRINT_WAVES; ++v) cmin_merge(best, best_e, red_c[v], red_e[v]);
    a.row_rec[(size_t)row * FOOTPRINT_ROW_REC] = best;
    a.row_rec[(size_t)row * FOOTPRINT_ROW_REC + 1] = best_e == NO_INDEX ? -1.0 : (double)best_e;
  }
}

constexpr int MAP_COLS = 4;  // columns whose loads are in flight together

// Lane `from`'s value (wavefront-uniform index) as a scalar.
__device__ __forceinline__ double lane_double(double v, int from) {
  const unsigned long long w = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)w, from), hi = __builtin_amdgcn_readlane((unsigned)(w >> 32), from);
  return __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

// (max occupancy, lowest cell)
__device__ __forceinline__ void occ_merge(float& o0, int& c0, float o1, int c1) {
  if (o1 > o0 || (o1 == o0 && c1 < c0)) { o0 = o1; c0 = c1; }
}

__global__ __launch_bounds__(FOOTPRINT_THREADS) void cilqr_footprint_map_kernel(FootprintArgs a) {
#pragma clang fp contract(off)  // cell centres and crossing abscissae as the rasteriser forms them
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int N = a.s.N, G = (N + FOOTPRINT_WAVES - 1) / FOOTPRINT_WAVES;
  const int row = blockIdx.x / G, t = (blockIdx.x - row * G) * FOOTPRINT_WAVES + wave;  // (wavefront-uniform)
  if (t >= N) return;  // (a workgroup's last wavefronts idle where N is no multiple of four; the kernel has no barrier)
  const int b = row / a.S;
  const double* X = a.X + ((size_t)row * ((size_t)N + 1) + t) * 4;
  const double x = X[0], y = X[1], th = X[3];
  bool lost = !(is_finite(x) && is_finite(y) && is_finite(th));
  double qx[4] = {0.0, 0.0, 0.0, 0.0}, qy[4] = {0.0, 0.0, 0.0, 0.0};
  FootprintRange r = {0, -1, 0, -1, 0};
  if (!lost) {
    double st, ct;
    sincos_fast(th, &st, &ct);
    const UncPose po = unc_pose(a.s.unc, b);
    footprint_corners(x, y, ct, st, a.hl, a.hw, po.px, po.py, po.cp, po.sp, qx, qy);
#pragma unroll
    for (int k = 0; k < 4; ++k) { qx[k] = uniform_double(qx[k]); qy[k] = uniform_double(qy[k]); }
    r = footprint_range(qx, qy, a.s.unc.x_first, a.s.unc.y_first, a.s.unc.inv_res);
    lost = !r.ok;  // (a footprint whose index range leaves ±2^30 is lost as a state that is not finite is)
  }

  int cells = 0, above = 0, max_c = NO_INDEX;
  bool unknown = false;
  float max_o = -__builtin_huge_valf();
  if (!lost) {
    const int rows = a.s.unc.rows, cols = a.s.unc.cols;
    const LayerPtr layer = (LayerPtr)(a.s.unc.layer + (size_t)b * (size_t)a.s.unc.stride);
    const double x_first = a.s.unc.x_first, y_first = a.s.unc.y_first, res = a.res, threshold = a.occ_threshold;
    // A chunk of 64 columns at a time.  First lane c decides column j0 + c: which edges straddle its row of centres and where they
    // cross it — Polygon::isInside's statements, the IEEE division among them, once per column and not once per cell.  Then the
    // columns are walked uniformly, their crossing abscissae read out of lane c into scalar registers, in groups of MAP_COLS: a
    // group's coverage is decided and its loads are issued before the first of them is used, so a wavefront waits for the layer
    // once per group (profiles/r22_footprint.txt).
    for (int j0 = r.j_lo; j0 <= r.j_hi; j0 += WAVE) {  // (uniform)
      const int jc = j0 + lane;
      const double py = y_first + res * (double)(-jc);
      unsigned straddles = 0;
      double at[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // edge k runs from vertex k - 1 (mod 4) to vertex k
        const double xi = qx[k], yi = qy[k], xj = qx[(k + 3) & 3], yj = qy[(k + 3) & 3];
        const bool straddle = (yi > py) != (yj > py);
        at[k] = straddle ? (xj - xi) * (py - yi) / (yj - yi) + xi : 0.0;
        straddles |= straddle ? 1u << k : 0u;
      }
      if (jc > r.j_hi) straddles = 0;
      const int n_cols = min(WAVE, r.j_hi - j0 + 1);
      for (int i0 = r.i_lo; i0 <= r.i_hi; i0 += WAVE) {
        const int i = i0 + lane;  // (at most 2^30 + 63)
        const double px = x_first + res * (double)(-i);
        const bool row_ok = i <= r.i_hi, row_in = i >= 0 && i < rows && row_ok;
        for (int c0 = 0; c0 < n_cols; c0 += MAP_COLS) {  // (uniform)
          float v[MAP_COLS];
          bool covered[MAP_COLS];
#pragma unroll
          for (int c = 0; c < MAP_COLS; ++c) {
            const int col = min(c0 + c, WAVE - 1), j = j0 + col;  // (a group's columns beyond the chunk straddle nothing: lane 63's, or none)
            const unsigned cross = c0 + c < n_cols ? (unsigned)__builtin_amdgcn_readlane((int)straddles, col) : 0u;
            bool odd = false;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (cross >> k & 1u) odd = odd != (px < lane_double(at[k], col));  // (uniform branch)
            covered[c] = odd && row_ok;
            v[c] = __builtin_nanf("");
            // (the only load of the layer: of a covered cell inside [0, rows) x [0, cols))
            if (covered[c] && row_in && j >= 0 && j < cols) v[c] = layer[(size_t)j * rows + i];
          }
#pragma unroll
          for (int c = 0; c < MAP_COLS; ++c) {
            if (covered[c]) {
              ++cells;
              if (v[c] == v[c]) {  // (so inside the map: i + j·rows is a cell of the layer, below 2^31)
                if (fabsf(v[c]) < 3.0e38f) occ_merge(max_o, max_c, v[c], i + (j0 + c0 + c) * rows);
                if ((double)v[c] > threshold) ++above;
              } else {
                unknown = true;  // outside the map, or NaN
              }
            }
          }
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    cells += __shfl_xor(cells, o, WAVE);
    above += __shfl_xor(above, o, WAVE);
    occ_merge(max_o, max_c, __shfl_xor(max_o, o, WAVE), __shfl_xor(max_c, o, WAVE));
  }
  const bool any_unknown = __ballot(unknown) != 0ull || lost;
  if (lane == 0) {
    const bool hits = lost || above > 0 || ((a.flags & CILQR_FOOTPRINT_UNKNOWN_HITS) && any_unknown);
    double* rec = a.steps + ((size_t)row * N + t) * FOOTPRINT_STEP_REC;
    rec[1] = max_c == NO_INDEX ? -__builtin_huge_val() : (double)max_o;
    rec[2] = max_c == NO_INDEX ? -1.0 : (double)max_c;
    rec[3] = (double)above;
    rec[4] = (double)((hits ? 1 : 0) | (any_unknown ? 2 : 0));
    rec[5] = (double)cells;
  }
}

// One wavefront per row: the N step records and the boxes' record → fp [CILQR_FOOTPRINT_FIELDS], step_occ and total.
__global__ __launch_bounds__(WAVE) void cilqr_footprint_merge_kernel(FootprintArgs a) {
  const int row = blockIdx.x, lane = threadIdx.x, N = a.s.N;
  const double* rec = a.steps + (size_t)row * N * FOOTPRINT_STEP_REC;
  float* step_occ = a.step_occ ? a.step_occ + (size_t)row * N : nullptr;
  int hit_steps = 0, first = NO_INDEX, map_hits = 0, map_first = NO_INDEX, most_above = 0, unknown_steps = 0;
  long long cells = 0;
  double max_o = -__builtin_huge_val();
  int max_t = NO_INDEX, max_c = NO_INDEX;
  for (int t = lane; t < N; t += WAVE) {
    const double* p = rec + (size_t)t * FOOTPRINT_STEP_REC;
    if (p[0] != 0.0) { ++hit_steps; first = min(first, t); }
    float occ = __builtin_nanf("");
    if (a.map_on) {
      const double o = p[1];
      const int c = (int)p[2], fl = (int)p[4];
      if (c >= 0) {
        occ = (float)o;
        if (o > max_o || (o == max_o && t < max_t)) { max_o = o; max_t = t; max_c = c; }
      }
      if (fl & 1) { ++map_hits; map_first = min(map_first, t); }
      if (fl & 2) ++unknown_steps;
      most_above = max(most_above, (int)p[3]);
      cells += (long long)p[5];
    }
    if (step_occ) step_occ[t] = occ;
  }
  for (int o = 32; o > 0; o >>= 1) {
    hit_steps += __shfl_xor(hit_steps, o, WAVE);
    first = min(first, __shfl_xor(first, o, WAVE));
    map_hits += __shfl_xor(map_hits, o, WAVE);
    map_first = min(map_first, __shfl_xor(map_first, o, WAVE));
    most_above = max(most_above, __shfl_xor(most_above, o, WAVE));
    unknown_steps += __shfl_xor(unknown_steps, o, WAVE);
    cells += __shfl_xor(cells, o, WAVE);
    const double o1 = __shfl_xor(max_o, o, WAVE);
    const int t1 = __shfl_xor(max_t, o, WAVE), c1 = __shfl_xor(max_c, o, WAVE);
    if (o1 > max_o || (o1 == max_o && t1 < max_t)) { max_o = o1; max_t = t1; max_c = c1; }
  }
  if (lane == 0) {
    const double clearance = a.row_rec[(size_t)row * FOOTPRINT_ROW_REC];
    double* out = a.fp + (size_t)row * CILQR_FOOTPRINT_FIELDS;
    out[CILQR_FP_CLEARANCE] = clearance;
    out[CILQR_FP_CLEARANCE_ENTRY] = a.row_rec[(size_t)row * FOOTPRINT_ROW_REC + 1];
    out[CILQR_FP_HIT_STEPS] = (double)hit_steps;
    out[CILQR_FP_FIRST_HIT] = first == NO_INDEX ? -1.0 : (double)first;
    out[CILQR_FP_MAP_OCC] = max_o;
    out[CILQR_FP_MAP_OCC_STEP] = max_t == NO_INDEX ? -1.0 : (double)max_t;
    out[CILQR_FP_MAP_OCC_CELL] = max_t == NO_INDEX ? -1.0 : (double)max_c;
    out[CILQR_FP_MAP_HIT_STEPS] = (double)map_hits;
    out[CILQR_FP_MAP_FIRST_HIT] = map_first == NO_INDEX ? -1.0 : (double)map_first;
    out[CILQR_FP_MAP_HIT_CELLS] = (double)most_above;
    out[CILQR_FP_MAP_UNKNOWN_STEPS] = (double)unknown_steps;
    out[CILQR_FP_MAP_CELLS] = (double)cells;
    if (a.total) {
      const double base = a.base[row];
      const bool clear = hit_steps == 0 && clearance >= a.min_clearance && map_hits == 0;
      a.total[row] = is_finite(base) && clear ? base : __builtin_nan("");
    }
  }
}

}  // namespace

size_t footprint_lds_bytes(int N) {
  return ((size_t)5 * N + FOOTPRINT_WAVES) * sizeof(double) + ((size_t)N + FOOTPRINT_WAVES) * sizeof(int32_t);
}

hipError_t launch_footprint_check(const FootprintArgs& a, hipStream_t stream) {
  if (a.rows <= 0 || a.s.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(cilqr_footprint_boxes_kernel, dim3(a.rows), dim3(FOOTPRINT_THREADS), footprint_lds_bytes(a.s.N), stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.map_on) {
    const long long blocks = (long long)a.rows * ((a.s.N + FOOTPRINT_WAVES - 1) / FOOTPRINT_WAVES);
    hipLaunchKernelGGL(cilqr_footprint_map_kernel, dim3((unsigned)blocks), dim3(FOOTPRINT_THREADS), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(cilqr_footprint_merge_kernel, dim3(a.rows), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
