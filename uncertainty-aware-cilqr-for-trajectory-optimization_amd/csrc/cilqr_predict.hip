// cilqr_predict.hip — tracked obstacles rolled out over the horizon with their covariance (cilqr_predict_obstacles*,
// include/cilqr.h): from one state (x, y, v, theta, a, omega) and one 4x4 covariance per vehicle the [4N] pose and [2N] dimension
// rows every obstacle-reading call takes, and P_t per step — the obs_cov of cilqr_tighten_obstacles and cilqr_chance_risk_cov.
//
// Mapping: one wavefront per track, T·M workgroups of 64 lanes.  A track's bits come from its own inputs and N alone.  Phases:
//   speeds   v_t and theta_t by their recurrences (two additions and a compare per step, every lane the same; lane t mod 64 keeps
//            step t's pair in LDS).  They are serial by definition: a braking vehicle stops at the step its speed would turn
//            negative.
//   stage    lane = step t (strided): a_t, adv, the sincos of the heading → the step's advance (dx, dy) = (cos, sin)·adv and the two
//            remaining entries of N_t = A_t - I, dt·cos and dt·sin; its other two are (-dy, dx).  The N sincos run side by side.
//   chain    x_t, y_t by summation and the ten row <= column entries of P_t by  P' = P + N P + P N' + N P N' + Q  written out for
//            the four non-zero entries of N_t: 20 fused multiply-adds and ten additions a step, every lane the same and all ten
//            entries in its own registers — no cross-lane move and no LDS round trip on the serial path; the step's four
//            coefficients leave LDS one step ahead.  Lane 0 stores x_t, y_t and the ten entries to LDS without waiting.
//   stores   lane = output element (strided), coalesced: poses, dimensions, cov_out's three entries, sigma_out's sixteen (mirrored
//            from the ten).
// What this mapping trades: all 64 lanes run the two serial passes (the speed recurrence and the chain) redundantly and lane 0 alone
// stores the chain's results, so a large T·M (4096 wavefronts at T = 1024, M = 4) spends 64 lanes of issue on one lane's work —
// throughput given up for a chain without a cross-lane move, which is what the planner's T·M <= 64 waits for.
// LDS (dynamic, doubles): [pose: 4·N][step: 4·N][P: 10·N] = 8·18·N bytes.
// No atomics, no scratch memory, no spilled register (make check).
#include "cilqr_device.hpp"

namespace cilqr {

using namespace dev;

namespace {

// Row <= column entry (r, c) of a symmetric 4x4 in the order 00 01 02 03 11 12 13 22 23 33.
__device__ __forceinline__ int upper_index(int r, int c) {
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return (lo == 0 ? 0 : lo == 1 ? 3 : lo == 2 ? 5 : 6) + hi;
}

__global__ __launch_bounds__(PREDICT_THREADS) void cilqr_predict_obstacles_kernel(PredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) double predict_lds[];
  const int lane = threadIdx.x, N = a.N;
  const size_t k = blockIdx.x;
  double* ps = predict_lds;            // [N][4]: x, y, v, theta
  double* st = ps + (size_t)4 * N;     // [N][4]: dx, dy, dt cos, dt sin
  double* cv = st + (size_t)4 * N;     // [N][10]: P_t, row <= column
  const double* tr = a.track + 6 * k;
  const double dt = a.dt, acc = tr[4];
  double adt, wdt;
  {
#pragma clang fp contract(off)
    adt = acc * dt;
    wdt = tr[5] * dt;
  }

  // ---- speeds and headings
  {
#pragma clang fp contract(off)
    double v = tr[2], th = tr[3];
    for (int t = 0; t < N; ++t) {
      if (lane == (t & (WAVE - 1))) { ps[4 * t + 2] = v; ps[4 * t + 3] = th; }
      const double vn = v + adt;
      v = vn < 0.0 ? 0.0 : vn;
      th = th + wdt;
    }
  }
  __syncthreads();

  // ---- stage: the step's advance and the entries of A_t - I
  {
#pragma clang fp contract(off)
    const double h2 = a.half_dt2;
    for (int t = lane; t < N; t += WAVE) {
      const double v = ps[4 * t + 2], th = ps[4 * t + 3];
      const double at = v + adt < 0.0 ? -v / dt : acc;
      const double adv = v * dt + at * h2;
      double sn, cs;
      sincos_fast(th, &sn, &cs);
      double* s = st + 4 * t;
      s[0] = cs * adv; s[1] = sn * adv; s[2] = dt * cs; s[3] = dt * sn;
    }
  }
  __syncthreads();

  // ---- chain: positions and P_0 → P_{N-1}
  {
    double p[10], q[10];
    {
      const double* c0 = a.track_cov ? a.track_cov + 16 * k : nullptr;
      int i = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = r; c < 4; ++c, ++i) {
          p[i] = c0 ? c0[r + 4 * c] : 0.0;
          q[i] = a.noise ? a.noise[r + 4 * c] : 0.0;
        }
    }
    double x = tr[0], y = tr[1];
    double dx = st[0], dy = st[1], n02 = st[2], n12 = st[3];
    for (int t = 0; t < N; ++t) {
      if (lane == 0) {
        ps[4 * t] = x; ps[4 * t + 1] = y;
        double* o = cv + (size_t)10 * t;
#pragma unroll
        for (int i = 0; i < 10; ++i) o[i] = p[i];
      }
      // the next step's coefficients leave LDS before this step's arithmetic (the last step re-reads its own)
      const double* sn = st + 4 * (t + 1 < N ? t + 1 : t);
      const double ndx = sn[0], ndy = sn[1], nn02 = sn[2], nn12 = sn[3];
      {
#pragma clang fp contract(off)
        x = x + dx;
        y = y + dy;
        // N_t: (0,2) = n02, (1,2) = n12, (0,3) = -dy, (1,3) = dx.  G = (I + N) P, then P' = G (I + N)' + Q.
        const double n03 = -dy, n13 = dx;
        const double g00 = __builtin_fma(n03, p[3], __builtin_fma(n02, p[2], p[0]));
        const double g01 = __builtin_fma(n03, p[6], __builtin_fma(n02, p[5], p[1]));
        const double g02 = __builtin_fma(n03, p[8], __builtin_fma(n02, p[7], p[2]));
        const double g03 = __builtin_fma(n03, p[9], __builtin_fma(n02, p[8], p[3]));
        const double g11 = __builtin_fma(n13, p[6], __builtin_fma(n12, p[5], p[4]));
        const double g12 = __builtin_fma(n13, p[8], __builtin_fma(n12, p[7], p[5]));
        const double g13 = __builtin_fma(n13, p[9], __builtin_fma(n12, p[8], p[6]));
        p[0] = __builtin_fma(n03, g03, __builtin_fma(n02, g02, g00)) + q[0];
        p[1] = __builtin_fma(n13, g03, __builtin_fma(n12, g02, g01)) + q[1];
        p[4] = __builtin_fma(n13, g13, __builtin_fma(n12, g12, g11)) + q[4];
        p[2] = g02 + q[2]; p[3] = g03 + q[3]; p[5] = g12 + q[5]; p[6] = g13 + q[6];
        p[7] = p[7] + q[7]; p[8] = p[8] + q[8]; p[9] = p[9] + q[9];
      }
      dx = ndx; dy = ndy; n02 = nn02; n12 = nn12;
    }
  }
  __syncthreads();

  // ---- stores
  {
    double* pose = a.pose_out + k * 4 * N;
    for (int i = lane; i < 4 * N; i += WAVE) pose[i] = ps[i];
    const double d0 = a.track_dim[2 * k], d1 = a.track_dim[2 * k + 1];
    double* dim = a.dim_out + k * 2 * N;
    for (int i = lane; i < 2 * N; i += WAVE) dim[i] = (i & 1) ? d1 : d0;
    if (a.cov_out) {
      double* out = a.cov_out + k * 3 * N;
      for (int i = lane; i < 3 * N; i += WAVE) {
        const int t = i / 3, j = i - 3 * t;
        out[i] = cv[(size_t)10 * t + (j == 2 ? 4 : j)];  // (0,0), (0,1), (1,1)
      }
    }
    if (a.sigma_out) {
      double* out = a.sigma_out + k * 16 * N;
      for (int i = lane; i < 16 * N; i += WAVE) out[i] = cv[(size_t)10 * (i >> 4) + upper_index(i & 3, (i >> 2) & 3)];
    }
  }
}

}  // namespace

size_t predict_lds_bytes(int N) { return (size_t)18 * N * sizeof(double); }

hipError_t launch_predict_obstacles(const PredictArgs& a, hipStream_t stream) {
  if (a.tracks <= 0) return hipSuccess;
  hipLaunchKernelGGL(cilqr_predict_obstacles_kernel, dim3((unsigned)a.tracks), dim3(PREDICT_THREADS), predict_lds_bytes(a.N), stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
