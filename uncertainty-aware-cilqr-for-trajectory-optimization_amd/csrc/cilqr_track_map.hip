// cilqr_track_map.hip — predicted tracks rasterised into the costmap along each plan (cilqr_rasterize_tracks*, include/cilqr.h): per
// solve a copy of the uncertainty-map layer set on the handle in which every cell is raised to 100 x the probability that a
// predicted vehicle covers it, taken at the steps when that solve's plan is near the cell (or, without a plan, over the whole
// horizon).  The result is one dense layer per solve that a warm-started re-solve reads.
//
// Three launches, no atomics, no arrival order in any result:
//   records  lane = entry e = m·N + t.  The entry's record — centre, cos and sin of its heading, the two half sizes, 1/(su·sqrt 2) and
//            1/(sw·sqrt 2), the two reaches — is a function of the track alone: not of the cell, the map pose or the solve.  With a
//            batch stride of 0 there is ONE set of M·N records per call, else one per solve.  They lie in device memory the handle
//            reserved at create; a lost entry's reach is -1, which no |du| meets.
//   cells    lane = cell.  Solve b has G workgroups of TRACK_MAP_THREADS lanes (G = min(ceil(cells / 256), TRACK_MAP_MAX_G) — a
//            function of the map alone, never of B) on a grid of B x G; workgroup g takes cells g·256 + lane, then steps by G·256.
//            Along a plan the N positions p_t go to LDS in the map frame (a lost step's p_t.x is NaN: it fails the search's `<`),
//            the search over t reads them at one address per wavefront, and the cell then meets (2·window + 1)·M records: 80 bytes
//            each, the 2·window + 1 of one track side by side.  Swept, every lane of the workgroup meets every record at the same
//            address.  The reach test comes first; the four erf are behind it.
//   finish   every wavefront reduces (raised count, (largest v, lowest cell, its entry)) by a butterfly, the first lane merges the
//            four records and leaves ONE per workgroup; one wavefront per solve merges the G of them and counts the lost entries.
//            Lexicographic maxima and integer counts: no order changes a bit, so neither does G.
// All arithmetic the definition states runs with contraction off: the header's formulas, evaluated as C evaluates them.
// LDS (dynamic, doubles): [pose: 4][steps: 2·N][records: 4·4] = 8·(2·N + 20) bytes.  No scratch memory, no spilled register (make check).
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int WAVES = TRACK_MAP_THREADS / WAVE;
constexpr double SQRT2 = 1.4142135623730951;
constexpr double SIGMA_MIN = 1e-150;  // a standard deviation below it counts as 0: its reciprocal would not be finite

__global__ __launch_bounds__(TRACK_MAP_THREADS) void cilqr_track_map_records_kernel(TrackMapArgs a) {
#pragma clang fp contract(off)
  const int N = a.s.N, E = a.s.M * N;
  const int chunks = (E + TRACK_MAP_THREADS - 1) / TRACK_MAP_THREADS;
  const int set = blockIdx.x / chunks, e = (blockIdx.x - set * chunks) * TRACK_MAP_THREADS + threadIdx.x;
  if (e >= E) return;
  const int m = e / N, t = e - m * N;
  const long long at = obs_entry_index(a.s, set, m, t);
  const double* pose = a.s.obs_pose + 4 * at;
  const double* dim = a.s.obs_dim + 2 * at;
  const double x = pose[0], y = pose[1], th = pose[3], len = dim[0], wid = dim[1];
  double cxx = 0.0, cxy = 0.0, cyy = 0.0;
  if (a.obs_cov) {
    const double* c3 = a.obs_cov + 3 * at;
    cxx = c3[0]; cxy = c3[1]; cyy = c3[2];
  }
  const bool live = is_finite(x) && is_finite(y) && is_finite(th) && is_finite(len) && is_finite(wid) && is_finite(cxx) &&
                    is_finite(cxy) && is_finite(cyy);
  double s, c;
  sincos(th, &s, &c);
  const double hl = (len + a.inflate) / 2.0, hw = (wid + a.inflate) / 2.0;
  const double cc = c * c, ss = s * s, cs = c * s;
  const double su2 = cc * cxx + 2.0 * cs * cxy + ss * cyy;
  const double sw2 = ss * cxx - 2.0 * cs * cxy + cc * cyy;
  const double su = sqrt(su2 < 0.0 ? 0.0 : su2), sw = sqrt(sw2 < 0.0 ? 0.0 : sw2);
  double* r = a.records + ((size_t)set * E + e) * TRACK_MAP_ENTRY;
  r[0] = x; r[1] = y; r[2] = c; r[3] = s; r[4] = hl; r[5] = hw;
  r[6] = su >= SIGMA_MIN ? 1.0 / (su * SQRT2) : 0.0;
  r[7] = sw >= SIGMA_MIN ? 1.0 / (sw * SQRT2) : 0.0;
  r[8] = live ? hl + a.z_max * su : -1.0;
  r[9] = live ? hw + a.z_max * sw : -1.0;
}

__global__ __launch_bounds__(TRACK_MAP_THREADS) void cilqr_track_map_kernel(TrackMapArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double track_map_lds[];
  const int tid = threadIdx.x;
  const int N = a.s.N;
  const int b = blockIdx.x, g = blockIdx.y;  // (the grid is B x G: both come free of a division and of a register to keep them in)
  const int cells = a.s.unc.rows * a.s.unc.cols;
  const bool along = a.X != nullptr;
  double* pose = track_map_lds;                           // px, py, cos, sin of the solve's map pose
  double* steps = pose + TRACK_MAP_POSE;                  // [N][TRACK_MAP_STEP]
  double* rec = steps + (size_t)TRACK_MAP_STEP * N;       // [WAVES][TRACK_MAP_REC]

  // ---- stage: the map pose, and p_t in the map frame
  {
    const UncPose po = unc_pose(a.s.unc, b);
    if (tid == 0) { pose[0] = po.px; pose[1] = po.py; pose[2] = po.cp; pose[3] = po.sp; }
    int lost = 0;
    if (along) {
      const double* X = a.X + (size_t)b * 4 * (N + 1);
      // (the trip count is the workgroup's, so that every lane meets the counting barrier; a lane beyond N stages nothing)
      for (int t0 = 0; t0 < N; t0 += TRACK_MAP_THREADS) {
        const int t = t0 + tid;
        bool is_lost = false;
        if (t < N) {
          const double x = X[4 * t], y = X[4 * t + 1];
          const bool live = is_finite(x) && is_finite(y);
          const double dx = x - po.px, dy = y - po.py;
          double* r = steps + (size_t)TRACK_MAP_STEP * t;
          r[0] = live ? po.cp * dx + po.sp * dy : __builtin_nan("");
          r[1] = po.cp * dy - po.sp * dx;
          is_lost = !live;
        }
        lost += __syncthreads_count(is_lost ? 1 : 0);
      }
    }
    __syncthreads();
    if (g == 0 && tid == 0) a.fields[(size_t)b * CILQR_TRACK_MAP_FIELDS + CILQR_TKM_LOST_STEPS] = (double)lost;
  }

  // ---- cells.  What a cell needs of the arguments is read where it is used, through a pointer the compiler cannot trace back to
  // the preloaded arguments, and the pose comes from LDS: erf's coefficients take some sixty scalar registers inside the entry loop,
  // and nothing else may be carried across it.
  int raised = 0, max_cell = NO_INDEX, max_entry = NO_INDEX;
  double max_v = 0.0;
  {
    const int first = g * TRACK_MAP_THREADS + tid;
    // (a 64-bit counter: near 2^31 cells the last step past the end does not fit an int)
    for (long long at = first; at < cells; at += (long long)kernel_args<TrackMapArgs>().G * TRACK_MAP_THREADS) {
      const TrackMapArgs& q = kernel_args<TrackMapArgs>();
      const int cell = (int)at, N = q.s.N;
      double wx, wy;
      int t_lo = 0, t_hi = N - 1;
      {
        const int rows = q.s.unc.rows;
        const int j = cell / rows, i = cell - j * rows;
        const double res = q.res;
        const double mx = q.s.unc.x_first - (double)i * res, my = q.s.unc.y_first - (double)j * res;
        if (q.X != nullptr) {
          // the nearest live step: strict <, so the lowest t on equal values; a NaN or infinite distance is never smaller
          int ts = -1;
          double best_d2 = __builtin_huge_val();
          for (int t = 0; t < N; ++t) {
            const double* r = steps + (size_t)TRACK_MAP_STEP * t;
            const double dx = mx - r[0], dy = my - r[1];
            const double d2 = dx * dx + dy * dy;
            if (d2 < best_d2) { best_d2 = d2; ts = t; }
          }
          // (window <= N: the sums stay inside an int.  No live step: an empty range)
          const int window = q.window;
          t_lo = ts < 0 ? 0 : (ts - window < 0 ? 0 : ts - window);
          t_hi = ts < 0 ? -1 : (ts + window > N - 1 ? N - 1 : ts + window);
        }
        const double px = pose[0], py = pose[1], cp = pose[2], sp = pose[3];
        wx = px + (cp * mx - sp * my);
        wy = py + (sp * mx + cp * my);
      }
      double best_p = 0.0;
      int best_e = NO_INDEX;
      {
        const int M = q.s.M;
        const bool bound_min = (q.flags & CILQR_TRACK_MAP_BOUND_MIN) != 0;
        const double* recs = q.records + (q.sets > 1 ? (size_t)b * (size_t)M * N * TRACK_MAP_ENTRY : (size_t)0);
        for (int m = 0; m < M; ++m) {
          const double* r = recs + ((size_t)m * N + t_lo) * TRACK_MAP_ENTRY;
          for (int t = t_lo; t <= t_hi; ++t, r += TRACK_MAP_ENTRY) {
            const double dx = wx - r[0], dy = wy - r[1];
            const double du = r[2] * dx + r[3] * dy, dw = r[2] * dy - r[3] * dx;
            if (fabs(du) <= r[8] && fabs(dw) <= r[9]) {
              // (ONE erf in a loop of four trips, not four side by side)
              const double hl = r[4], hw = r[5], ku = r[6], kw = r[7];
              double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
#pragma unroll 1
              for (int k = 0; k < 4; ++k) {
                const double arg = k == 0 ? (du + hl) * ku : k == 1 ? (du - hl) * ku : k == 2 ? (dw + hw) * kw : (dw - hw) * kw;
                const double f = erf(arg);
                e0 = k == 0 ? f : e0; e1 = k == 1 ? f : e1; e2 = k == 2 ? f : e2; e3 = k == 3 ? f : e3;
              }
              const double pu = ku > 0.0 ? 0.5 * (e0 - e1) : (fabs(du) <= hl ? 1.0 : 0.0);
              const double pw = kw > 0.0 ? 0.5 * (e2 - e3) : (fabs(dw) <= hw ? 1.0 : 0.0);
              const double p = bound_min ? (pw < pu ? pw : pu) : pu * pw;
              if (p > best_p) { best_p = p; best_e = m * N + t; }  // (entries ascend: the lowest on equal values stays)
            }
          }
        }
      }
      const size_t cells_ = (size_t)q.s.unc.rows * (size_t)q.s.unc.cols;
      const float own = (q.s.unc.layer + (size_t)b * (size_t)q.s.unc.stride)[cell];
      const float v = (float)(100.0 * best_p);
      float o = own;
      if (v > 0.0f && (own != own || own < v)) {
        o = v;
        ++raised;
      }
      if (v > 0.0f) row_merge(max_v, max_cell, max_entry, (double)v, cell, best_e);
      (q.layer_out + (size_t)b * cells_)[cell] = o;
    }
  }

  // ---- the workgroup's record: a butterfly per wavefront, then the first lane over the wavefronts' records
  const int lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  wave_row_merge(max_v, max_cell, max_entry);
  raised = wave_sum_int(raised);
  if (lane == 0) {
    double* r = rec + TRACK_MAP_REC * wave;
    r[0] = (double)raised; r[1] = max_v; r[2] = (double)max_cell; r[3] = (double)max_entry;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < WAVES; ++w) {
    const double* r = rec + TRACK_MAP_REC * w;
    raised += (int)r[0];
    row_merge(max_v, max_cell, max_entry, r[1], (int)r[2], (int)r[3]);
  }
  const TrackMapArgs& q = kernel_args<TrackMapArgs>();
  double* p = q.partials + ((size_t)b * q.G + g) * TRACK_MAP_REC;
  p[0] = (double)raised; p[1] = max_v; p[2] = (double)max_cell; p[3] = (double)max_entry;
}

// One wavefront per solve: the G workgroup records and the lost entries → fields (TKM_LOST_STEPS is the main kernel's).
__global__ __launch_bounds__(WAVE) void cilqr_track_map_finish_kernel(TrackMapArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, G = a.G, E = a.s.M * a.s.N;
  const double* part = a.partials + (size_t)b * G * TRACK_MAP_REC;
  const double* recs = a.records + (a.sets > 1 ? (size_t)b * (size_t)E * TRACK_MAP_ENTRY : (size_t)0);
  long long raised = 0;
  int max_cell = NO_INDEX, max_entry = NO_INDEX, lost = 0;
  double max_v = 0.0;
  for (int g = lane; g < G; g += WAVE) {
    const double* r = part + (size_t)TRACK_MAP_REC * g;
    raised += (long long)r[0];
    row_merge(max_v, max_cell, max_entry, r[1], (int)r[2], (int)r[3]);
  }
  for (int e = lane; e < E; e += WAVE) lost += recs[(size_t)e * TRACK_MAP_ENTRY + 8] < 0.0 ? 1 : 0;
  wave_row_merge(max_v, max_cell, max_entry);
  lost = wave_sum_int(lost);
  for (int o = 32; o > 0; o >>= 1) raised += __shfl_xor(raised, o, WAVE);
  if (lane == 0) {
    double* out = a.fields + (size_t)b * CILQR_TRACK_MAP_FIELDS;
    out[CILQR_TKM_RAISED] = (double)raised;
    out[CILQR_TKM_MAX_VALUE] = max_v;
    out[CILQR_TKM_MAX_CELL] = max_cell == NO_INDEX ? -1.0 : (double)max_cell;
    out[CILQR_TKM_MAX_ENTRY] = max_entry == NO_INDEX ? -1.0 : (double)max_entry;
    out[CILQR_TKM_LOST_ENTRIES] = (double)lost;
  }
}

}  // namespace

size_t track_map_lds_bytes(int N) { return (TRACK_MAP_POSE + (size_t)TRACK_MAP_STEP * N + TRACK_MAP_REC * WAVES) * sizeof(double); }

hipError_t launch_rasterize_tracks(const TrackMapArgs& a, hipStream_t stream) {
  if (a.s.B <= 0) return hipSuccess;
  const long long E = (long long)a.s.M * a.s.N;
  const long long chunks = (E + TRACK_MAP_THREADS - 1) / TRACK_MAP_THREADS;
  hipLaunchKernelGGL(cilqr_track_map_records_kernel, dim3((unsigned)(chunks * a.sets)), dim3(TRACK_MAP_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_track_map_kernel, dim3((unsigned)a.s.B, (unsigned)a.G), dim3(TRACK_MAP_THREADS), track_map_lds_bytes(a.s.N), stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_track_map_finish_kernel, dim3(a.s.B), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
