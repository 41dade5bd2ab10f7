// cilqr_tighten.hip — chance-constraint tightening of the obstacle table (cilqr_tighten_obstacles*, include/cilqr.h): every obstacle
// entry's (length, width) grown by kappa standard deviations of the relative position ego circle - obstacle along the ellipse's own
// axes, from the Σ_t that cilqr_chance_risk left in sigma_out.  The result is a dense table a warm-started re-solve reads.
//
// Mapping: one workgroup per solve, 64·min(4, ceil(max(N, M·N)/64)) lanes — a function of (N, M) alone.  Two phases:
//   stage    lane = step t (strided): the six entries of Σ_t the definition reads and sincos_fast of the heading → the position
//            covariance (xx, xy, yy) of the front and of the rear circle centre, 6 doubles per step in LDS.  What depends on the
//            step alone is formed N times, not M·N times.
//   entries  lane = obstacle entry e = m·N + t (strided): pose and dimensions through the strides of cilqr_obstacles, sincos of
//            the obstacle's heading (make_obs_entry's call, so the axes are the solver's), obs_cov added, the two axis variances
//            per circle, the larger of each, Δa and Δb with the cap; dim_out and the bit copy of the pose leave in entry order.
//   then     every wavefront reduces (max Δa, max Δb, (max of the larger Δ, lowest entry), capped count) by a butterfly, lane 0
//            of each leaves them in LDS, and the first lane of the workgroup merges the at most four records.  Maxima and an
//            integer count: no order of evaluation changes a bit.
// LDS (dynamic, doubles): [C: 6·N][records: 5·4] = 8·(6·N + 20) bytes.
// No scratch memory, no spilled register (make check).
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int RECORD = 5;  // doubles a wavefront leaves for the merge

// The larger of two variances, a NaN losing to a number, and not below 0; NaN when both are.
__device__ __forceinline__ double larger_variance(double f, double r) {
  const double m = fmax(f, r);
  return m < 0.0 ? 0.0 : m;
}

__global__ __launch_bounds__(TIGHTEN_THREADS) void cilqr_tighten_obstacles_kernel(TightenArgs a) {
  extern __shared__ __attribute__((aligned(16))) double tighten_lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE), waves = threads / WAVE;
  const int N = a.s.N, M = a.s.M, b = blockIdx.x;
  double* Cm = tighten_lds;              // [N][6]: front (xx, xy, yy), rear (xx, xy, yy)
  double* rec = Cm + (size_t)6 * N;      // [4][RECORD]

  // ---- stage: the circle centres' position covariances
  {
    const double* X = a.X + (size_t)b * 4 * (N + 1);
    const double* sig = a.sigma + (size_t)b * 16 * (N + 1);
    const double lever[2] = {a.s.kp.ego_front, -a.s.kp.ego_rear};
    for (int t = tid; t < N; t += threads) {
      const double* S = sig + (size_t)16 * t;  // entry (r, c) at [r + 4c], r <= c
      const double s00 = S[0], s01 = S[4], s03 = S[12], s11 = S[5], s13 = S[13], s33 = S[15];
      double sn, cs;
      sincos_fast(X[4 * t + 3], &sn, &cs);
      double* c = Cm + (size_t)6 * t;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double jx = -lever[k] * sn, jy = lever[k] * cs;
        c[3 * k] = s00 + 2.0 * jx * s03 + jx * jx * s33;
        c[3 * k + 1] = s01 + jx * s13 + jy * s03 + jx * jy * s33;
        c[3 * k + 2] = s11 + 2.0 * jy * s13 + jy * jy * s33;
      }
    }
  }
  __syncthreads();

  // ---- entries
  double max_da = 0.0, max_db = 0.0, max_v = -1.0;
  int max_e = NO_INDEX, capped = 0;
  {
    const int n_ent = M * N;
    const double kappa = a.kappa, cap = a.max_inflate;
    double* dim_out = a.dim_out + (size_t)b * 2 * n_ent;
    double* pose_out = a.pose_out ? a.pose_out + (size_t)b * 4 * n_ent : nullptr;
    for (int e = tid; e < n_ent; e += threads) {
      const int m = e / N, t = e - m * N;
      const long long at = obs_entry_index(a.s, b, m, t);
      const double* pose = a.s.obs_pose + 4 * at;
      const double* dim = a.s.obs_dim + 2 * at;
      const double p0 = pose[0], p1 = pose[1], p2 = pose[2], p3 = pose[3];
      double oxx = 0.0, oxy = 0.0, oyy = 0.0;
      if (a.obs_cov) { const double* oc = a.obs_cov + 3 * at; oxx = oc[0]; oxy = oc[1]; oyy = oc[2]; }
      double so, co;
      sincos(p3, &so, &co);
      const double cc = co * co, ss = so * so, cs2 = 2.0 * co * so;
      const double* c = Cm + (size_t)6 * t;
      const double fxx = c[0] + oxx, fxy = c[1] + oxy, fyy = c[2] + oyy;
      const double rxx = c[3] + oxx, rxy = c[4] + oxy, ryy = c[5] + oyy;
      const double va = larger_variance(cc * fxx + cs2 * fxy + ss * fyy, cc * rxx + cs2 * rxy + ss * ryy);
      const double vb = larger_variance(ss * fxx - cs2 * fxy + cc * fyy, ss * rxx - cs2 * rxy + cc * ryy);
      double da = kappa * sqrt(va), db = kappa * sqrt(vb);
      const bool ca = !is_finite(da) || da > cap, cb = !is_finite(db) || db > cap;
      da = ca ? cap : da;
      db = cb ? cap : db;
      capped += ca || cb ? 1 : 0;
      dim_out[2 * (size_t)e] = dim[0] + 2.0 * da;
      dim_out[2 * (size_t)e + 1] = dim[1] + 2.0 * db;
      if (pose_out) {
        double* po = pose_out + 4 * (size_t)e;
        po[0] = p0; po[1] = p1; po[2] = p2; po[3] = p3;
      }
      max_da = fmax(max_da, da);
      max_db = fmax(max_db, db);
      cmax_merge(max_v, max_e, fmax(da, db), e);
    }
  }

  // ---- the fields: a butterfly per wavefront, then the first lane over the wavefronts' records
  for (int o = 32; o > 0; o >>= 1) {
    max_da = fmax(max_da, __shfl_xor(max_da, o, WAVE));
    max_db = fmax(max_db, __shfl_xor(max_db, o, WAVE));
    const double ov = __shfl_xor(max_v, o, WAVE);
    const int oe = __shfl_xor(max_e, o, WAVE);
    cmax_merge(max_v, max_e, ov, oe);
    capped += __shfl_xor(capped, o, WAVE);
  }
  if (lane == 0) {
    double* r = rec + RECORD * wave;
    r[0] = max_da; r[1] = max_db; r[2] = max_v; r[3] = (double)max_e; r[4] = (double)capped;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < waves; ++w) {
    const double* r = rec + RECORD * w;
    max_da = fmax(max_da, r[0]);
    max_db = fmax(max_db, r[1]);
    cmax_merge(max_v, max_e, r[2], (int)r[3]);
    capped += (int)r[4];
  }
  double* out = a.tighten + (size_t)b * CILQR_TIGHTEN_FIELDS;
  out[CILQR_TG_MAX_DA] = max_da;
  out[CILQR_TG_MAX_DB] = max_db;
  out[CILQR_TG_MAX_ENTRY] = max_e == NO_INDEX ? -1.0 : (double)max_e;
  out[CILQR_TG_CAPPED] = (double)capped;
}

}  // namespace

size_t tighten_lds_bytes(int N) { return ((size_t)6 * N + RECORD * (TIGHTEN_THREADS / WAVE)) * sizeof(double); }

hipError_t launch_tighten_obstacles(const TightenArgs& a, hipStream_t stream) {
  if (a.s.B <= 0) return hipSuccess;
  const long long work = (long long)a.s.N * (a.s.M > 1 ? a.s.M : 1);
  const long long waves = (work + WAVE - 1) / WAVE;
  const int threads = WAVE * (int)(waves < TIGHTEN_THREADS / WAVE ? waves : TIGHTEN_THREADS / WAVE);
  hipLaunchKernelGGL(cilqr_tighten_obstacles_kernel, dim3((unsigned)a.s.B), dim3(threads), tighten_lds_bytes(a.s.N), stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
