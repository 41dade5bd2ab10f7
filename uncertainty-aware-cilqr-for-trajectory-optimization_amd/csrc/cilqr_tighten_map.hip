// cilqr_tighten_map.hip — map tightening (cilqr_tighten_map*, include/cilqr.h): the uncertainty-map layer set on the handle
// dilated, per cell, by kappa standard deviations of where the footprint point over that cell may really be, from the Sigma_t that
// cilqr_chance_risk left in sigma_out.  The result is one dense layer per solve that a warm-started re-solve reads.
//
// Mapping: lane = cell.  Solve b has G workgroups of TIGHTEN_MAP_THREADS lanes (G = min(ceil(cells / 256), TIGHTEN_MAP_MAX_G) — a
// function of the map alone, never of B); workgroup g takes cells g·256 + lane, then steps by G·256.  Three phases:
//   stage    lane = step t (strided): p_t and the six covariance entries turned into the map frame, 8 doubles per step in LDS (a
//            lost step's p_t.x is NaN: it fails the search's `<`; TM_LOST is counted at a barrier from the test of the inputs,
//            not from what p_t came to).  Every workgroup of a solve stages the same N records: 48 flops a step against the
//            N·256 distance tests that follow.
//   cells    the search over t reads LDS at one address per wavefront (a broadcast); then the cell's covariance, its reach, and the
//            gather over at most (2·ni + 1)·(2·nj + 1) cells of the INPUT layer — 60 KB at 150 x 100, resident in L2; the output
//            is another buffer, so no cell read here is one written here.
//   records  every wavefront reduces (raised count, (largest raise, lowest cell), largest reach, capped count) by a butterfly, the
//            first lane merges the at most four records and leaves ONE per workgroup in the handle's memory; the finish kernel,
//            one wavefront per solve, merges the G of them.  Lexicographic maxima and integer counts: no order changes a bit, so
//            neither does G.
// All arithmetic the definition states runs with contraction off: the header's formulas, evaluated as C evaluates them.
// LDS (dynamic, doubles): [steps: 8·N][records: 5·4] = 8·(8·N + 20) bytes.  No scratch memory, no spilled register (make check).
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int WAVES = TIGHTEN_MAP_THREADS / WAVE;

__device__ __forceinline__ bool finite_cell(float v) { return fabsf(v) <= 3.4028234663852886e38f; }  // (NaN fails the comparison)

__global__ __launch_bounds__(TIGHTEN_MAP_THREADS) void cilqr_tighten_map_kernel(TightenMapArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double tighten_map_lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int N = a.s.N, G = a.G;
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int rows = a.s.unc.rows, cols = a.s.unc.cols, cells = rows * cols;
  double* steps = tighten_map_lds;                          // [N][TIGHTEN_MAP_STEP]
  double* rec = steps + (size_t)TIGHTEN_MAP_STEP * N;       // [WAVES][TIGHTEN_MAP_REC]

  // ---- stage: p_t and the covariance entries in the map frame
  int lost = 0;
  {
    const UncPose po = unc_pose(a.s.unc, b);
    const double cp = po.cp, sp = po.sp;
    const double cc = cp * cp, ss = sp * sp, cs = cp * sp;
    const double* X = a.X + (size_t)b * 4 * (N + 1);
    const double* sig = a.sigma + (size_t)b * 16 * (N + 1);
    // (the trip count is the workgroup's, so that every lane meets the counting barrier; a lane beyond N stages nothing)
    for (int t0 = 0; t0 < N; t0 += TIGHTEN_MAP_THREADS) {
      const int t = t0 + tid;
      bool is_lost = false;
      if (t < N) {
        const double* S = sig + (size_t)16 * t;  // entry (r, c) at [r + 4c], r <= c
        const double x = X[4 * t], y = X[4 * t + 1], th = X[4 * t + 3];
        const double s00 = S[0], s01 = S[4], s11 = S[5], s03 = S[12], s13 = S[13], s33 = S[15];
        const bool live = is_finite(x) && is_finite(y) && is_finite(th) && is_finite(s00) && is_finite(s01) && is_finite(s11) &&
                          is_finite(s03) && is_finite(s13) && is_finite(s33);
        const double dx = x - po.px, dy = y - po.py;
        double* r = steps + (size_t)TIGHTEN_MAP_STEP * t;
        r[0] = live ? cp * dx + sp * dy : __builtin_nan("");
        r[1] = cp * dy - sp * dx;
        r[2] = cc * s00 + 2.0 * cs * s01 + ss * s11;
        r[3] = cs * (s11 - s00) + (cc - ss) * s01;
        r[4] = ss * s00 - 2.0 * cs * s01 + cc * s11;
        r[5] = cp * s03 + sp * s13;
        r[6] = cp * s13 - sp * s03;
        r[7] = s33;
        is_lost = !live;
      }
      lost += __syncthreads_count(is_lost ? 1 : 0);  // lost by the definition's test of the inputs, not by what p_t came to
    }
  }
  __syncthreads();
  if (g == 0 && tid == 0) a.tighten[(size_t)b * CILQR_TIGHTEN_MAP_FIELDS + CILQR_TM_LOST] = (double)lost;

  // ---- cells
  int raised = 0, capped = 0, max_cell = NO_INDEX;
  double max_raise = 0.0, max_reach = 0.0;
  {
    const float* in = a.s.unc.layer + (size_t)b * (size_t)a.s.unc.stride;
    float* out = a.layer_out + (size_t)b * (size_t)cells;
    const double res = a.res, r_fp = a.r_fp, kappa = a.kappa, cap = a.max_inflate;
    const double x_first = a.s.unc.x_first, y_first = a.s.unc.y_first;
    // (a 64-bit counter: near 2^31 cells the last step past the end does not fit an int)
    for (long long at = (long long)g * TIGHTEN_MAP_THREADS + tid; at < cells; at += (long long)G * TIGHTEN_MAP_THREADS) {
      const int cell = (int)at;
      const int j = cell / rows, i = cell - j * rows;
      const double mx = x_first - (double)i * res, my = y_first - (double)j * res;
      // the nearest live step: strict <, so the lowest t on equal values; a NaN or infinite distance is never smaller
      int ts = -1;
      double best_d2 = __builtin_huge_val();
      for (int t = 0; t < N; ++t) {
        const double* r = steps + (size_t)TIGHTEN_MAP_STEP * t;
        const double dx = mx - r[0], dy = my - r[1];
        const double d2 = dx * dx + dy * dy;
        if (d2 < best_d2) { best_d2 = d2; ts = t; }
      }
      const float own = in[cell];
      float best = own;
      if (ts >= 0) {
        const double* r = steps + (size_t)TIGHTEN_MAP_STEP * ts;
        double dx = mx - r[0], dy = my - r[1];
        const double len = sqrt(dx * dx + dy * dy);
        if (len > r_fp) {
          const double f = r_fp / len;
          dx = dx * f; dy = dy * f;
        }
        const double jx = -dy, jy = dx;
        const double pxx = r[2], pxy = r[3], pyy = r[4], cx = r[5], cy = r[6], stt = r[7];
        const double Cxx = pxx + 2.0 * jx * cx + jx * jx * stt;
        const double Cyy = pyy + 2.0 * jy * cy + jy * jy * stt;
        const double Cxy = pxy + jx * cy + jy * cx + jx * jy * stt;
        double hx = kappa * sqrt(Cxx < 0.0 ? 0.0 : Cxx), hy = kappa * sqrt(Cyy < 0.0 ? 0.0 : Cyy);
        const bool capx = !is_finite(hx) || hx > cap, capy = !is_finite(hy) || hy > cap;
        hx = capx ? cap : hx;
        hy = capy ? cap : hy;
        capped += capx || capy ? 1 : 0;
        max_reach = fmax(max_reach, fmax(hx, hy));
        if (finite_cell(own)) {
          const double fi = floor(hx / res), fj = floor(hy / res);
          const int ni = fi < (double)(rows - 1) ? (int)fi : rows - 1, nj = fj < (double)(cols - 1) ? (int)fj : cols - 1;
          const int a0 = -ni < -i ? -i : -ni, a1 = ni > rows - 1 - i ? rows - 1 - i : ni;
          const int b0 = -nj < -j ? -j : -nj, b1 = nj > cols - 1 - j ? cols - 1 - j : nj;
          const double det = Cxx * Cyy - Cxy * Cxy, lim = kappa * kappa * det;
          const bool box_only = !(det > 0.0);
          for (int bb = b0; bb <= b1; ++bb) {
            const double ey = -(double)bb * res;
            const float* col = in + (size_t)(j + bb) * rows + i;
            for (int aa = a0; aa <= a1; ++aa) {
              const double ex = -(double)aa * res;
              const double q = Cyy * (ex * ex) - 2.0 * Cxy * ex * ey + Cxx * (ey * ey);
              const float v = col[aa];
              if ((box_only || q <= lim) && finite_cell(v) && v > best) best = v;
            }
          }
          const double raise = (double)best - (double)own;
          if (raise > 0.0) {
            ++raised;
            cmax_merge(max_raise, max_cell, raise, cell);
          }
        }
      }
      out[cell] = best;
    }
  }

  // ---- the workgroup's record: a butterfly per wavefront, then the first lane over the wavefronts' records
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(max_raise, o, WAVE);
    const int oc = __shfl_xor(max_cell, o, WAVE);
    cmax_merge(max_raise, max_cell, ov, oc);
    max_reach = fmax(max_reach, __shfl_xor(max_reach, o, WAVE));
    raised += __shfl_xor(raised, o, WAVE);
    capped += __shfl_xor(capped, o, WAVE);
  }
  if (lane == 0) {
    double* r = rec + TIGHTEN_MAP_REC * wave;
    r[0] = (double)raised; r[1] = max_raise; r[2] = (double)max_cell; r[3] = max_reach; r[4] = (double)capped;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < WAVES; ++w) {
    const double* r = rec + TIGHTEN_MAP_REC * w;
    raised += (int)r[0];
    cmax_merge(max_raise, max_cell, r[1], (int)r[2]);
    max_reach = fmax(max_reach, r[3]);
    capped += (int)r[4];
  }
  double* p = a.partials + ((size_t)b * G + g) * TIGHTEN_MAP_REC;
  p[0] = (double)raised; p[1] = max_raise; p[2] = (double)max_cell; p[3] = max_reach; p[4] = (double)capped;
}

// One wavefront per solve: the G workgroup records → tighten [CILQR_TIGHTEN_MAP_FIELDS] (TM_LOST is the main kernel's).
__global__ __launch_bounds__(WAVE) void cilqr_tighten_map_finish_kernel(TightenMapArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, G = a.G;
  const double* part = a.partials + (size_t)b * G * TIGHTEN_MAP_REC;
  long long raised = 0, capped = 0;
  int max_cell = NO_INDEX;
  double max_raise = 0.0, max_reach = 0.0;
  for (int g = lane; g < G; g += WAVE) {
    const double* r = part + (size_t)TIGHTEN_MAP_REC * g;
    raised += (long long)r[0];
    cmax_merge(max_raise, max_cell, r[1], (int)r[2]);
    max_reach = fmax(max_reach, r[3]);
    capped += (long long)r[4];
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(max_raise, o, WAVE);
    const int oc = __shfl_xor(max_cell, o, WAVE);
    cmax_merge(max_raise, max_cell, ov, oc);
    max_reach = fmax(max_reach, __shfl_xor(max_reach, o, WAVE));
    raised += __shfl_xor(raised, o, WAVE);
    capped += __shfl_xor(capped, o, WAVE);
  }
  if (lane == 0) {
    double* out = a.tighten + (size_t)b * CILQR_TIGHTEN_MAP_FIELDS;
    out[CILQR_TM_RAISED] = (double)raised;
    out[CILQR_TM_MAX_RAISE] = max_raise;
    out[CILQR_TM_MAX_CELL] = max_cell == NO_INDEX ? -1.0 : (double)max_cell;
    out[CILQR_TM_MAX_REACH] = max_reach;
    out[CILQR_TM_CAPPED] = (double)capped;
  }
}

}  // namespace

size_t tighten_map_lds_bytes(int N) { return ((size_t)TIGHTEN_MAP_STEP * N + TIGHTEN_MAP_REC * WAVES) * sizeof(double); }

hipError_t launch_tighten_map(const TightenMapArgs& a, hipStream_t stream) {
  if (a.s.B <= 0) return hipSuccess;
  const long long blocks = (long long)a.s.B * a.G;
  hipLaunchKernelGGL(cilqr_tighten_map_kernel, dim3((unsigned)blocks), dim3(TIGHTEN_MAP_THREADS), tighten_map_lds_bytes(a.s.N), stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_tighten_map_finish_kernel, dim3(a.s.B), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
