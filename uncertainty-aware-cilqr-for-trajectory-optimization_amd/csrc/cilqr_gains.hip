// cilqr_gains.hip — the feedback gains of ONE backward pass at a given trajectory (cilqr_gains_batch*, include/cilqr.h):
// iLQR::backward_pass(X, U, coeffs, x_plan, lamb), I/iLQR.cpp:91-195.  A solve returns U alone; this hands out the k_t, K_t its passes
// compute and drop, so that a plan can be tracked from a start other than the one it was solved for (cilqr_rollout.hip).
//
// Mapping: one wavefront per solve, the structure of one iteration of the one-wavefront solve family.
//   phase 0  lanes over the path samples → LDS (sample_xy); lanes over the states t ≤ N: cos/sin of the heading → LDS
//   phase L  lanes over the steps t < N: closest path sample (closest_sample: the strict-< first minimum), lin_step with the obstacle
//            entries read through the strides (obs_entry_at) — SAMPLED: entry m = o·n_samples + s made from nominal obstacle o and
//            sample s's offset by the plain additions of score_entry<true> (cilqr_score.hip), in ascending m, so that the record
//            carries the bits of the call on the materialised obstacles — the map term (unc_cost_add) in a loop of its own; the
//            record → LDS.
//            A and B are evaluated at state t + 1, as the reference does (I/iLQR.cpp:102-106).
//   phase R  lane 0 runs the serial chain riccati_step<false> — the branching form, which clamps negative eigenvalues as the
//            reference's EigenSolver path does, so that no solve is ever handed to another kernel — and stores each step's gains as
//            the chain produces them.  A step whose Q_uu is not finite ends the chain: ok = 0, and the gains from that step down to
//            step 0 are zero, as the reference leaves them (k, K are zero-initialised there and the loop breaks).
// The chain is one lane and serial by nature: there is no matrix-core variant here.
#include "cilqr_device.hpp"

namespace cilqr {

using namespace dev;

namespace {

struct LdsPath {  // the path samples as closest_sample reads them
  const double* sx;
  const double* sy;
  __device__ __forceinline__ void operator()(int s, double& x, double& y) const { x = sx[s]; y = sy[s]; }
};

// LDS (dynamic): [sx S][sy S][cos N+1][sin N+1][N records of REC_W doubles]
constexpr int REC_W = 16;

template <bool SAMPLED>
__global__ __launch_bounds__(WAVE) void cilqr_gains_kernel(GainsArgs a) {
  extern __shared__ double lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int N = a.s.N, S = a.s.kp.n_samples;
  double* sx = lds;
  double* sy = sx + S;
  double* ect = sy + S;
  double* est = ect + (N + 1);
  double* rec = est + (N + 1);
  const double* X = a.s.X_out + (size_t)b * 4 * (N + 1);
  const double* U = a.s.U + (size_t)b * 2 * N;

  // ---- phase 0
  SampleGrid grid;
  {
    const SolveArgs& s = phase_args();
    const double* pc = s.poly + (size_t)b * CILQR_POLY_COEFFS;
    make_sample_grid(grid, s.xplan_fl[2 * (size_t)b], s.xplan_fl[2 * (size_t)b + 1], S);
    for (int i = lane; i < S; i += WAVE) sample_xy(grid, pc, i, sx[i], sy[i]);
    for (int t = lane; t <= N; t += WAVE) sincos_fast(X[4 * t + 3], &est[t], &ect[t]);
  }
  __syncthreads();

  // ---- phase L: one record per step
  {
    const SolveArgs& s = phase_args();
    const KParams& kp = s.kp;
    const double* wts = SAMPLED ? nullptr : obs_weights(s, b);
    const int M = SAMPLED ? s.M * s.n_samples : s.M;  // (SAMPLED: s.M counts the nominal obstacles)
    for (int t = lane; t < N; t += WAVE) {
      const double px = X[4 * t], py = X[4 * t + 1];
      const int cs = closest_sample<false>(S, grid, px, py, LdsPath{sx, sy});
      auto obs = [&](int m, ObsEntry& e, double& w) {
        if (SAMPLED) {  // the pose the materialised call is given: (x + dx, y + dy, v, theta + dtheta)
          const int o = m / s.n_samples;
          const long long ob = (long long)b * s.M + o, en = ob * N + t;
          const double* np = s.obs_pose + 4 * en;
          const double* off = s.samp_off + 3 * (ob * s.n_samples + (m - o * s.n_samples));
          const double pose[4] = {np[0] + off[0], np[1] + off[1], np[2], np[3] + off[2]};
          e = make_obs_entry(kp, pose, s.obs_dim + 2 * en);
          w = s.samp_w;
          return true;
        }
        e = obs_entry_at(kp, s, b, m, t);
        w = wts ? wts[m] : kp.w_obstacle;
        return true;
      };
      Rec c;
      lin_step(kp, px, py, X[4 * t + 2], ect[t], est[t], U[2 * t], U[2 * t + 1], X[4 * (t + 1) + 2], ect[t + 1], est[t + 1], sx[cs], sy[cs],
               M, obs, c);
      double* r = rec + (size_t)t * REC_W;
      r[0] = c.lx0; r[1] = c.lx1; r[2] = c.lx2; r[3] = c.l00; r[4] = c.l01; r[5] = c.l11;
      r[6] = c.lu0; r[7] = c.lu1; r[8] = c.luu0; r[9] = c.luu1;
      r[10] = c.al; r[11] = c.be; r[12] = c.ga; r[13] = c.de; r[14] = c.p; r[15] = c.q;
    }
  }
  // the map term, added to the stored records after the obstacle terms (the reference's order of summation), in a loop of its own
  if (phase_args().unc.layer) {
    const UncArgs& u = phase_args().unc;
    const UncPose po = unc_pose(u, b);
    for (int t = lane; t < N; t += WAVE) {
      double* r = rec + (size_t)t * REC_W;
      double lx0 = r[0], lx1 = r[1], l00 = r[3], l01 = r[4], l11 = r[5];
      unc_cost_add(u, po, b, X[4 * t], X[4 * t + 1], ect[t], est[t], lx0, lx1, l00, l01, l11);
      r[0] = lx0; r[1] = lx1; r[3] = l00; r[4] = l01; r[5] = l11;
    }
  }
  __syncthreads();

  // ---- phase R: the serial chain on one lane
  if (lane == 0) {
    const GainsArgs& g = *reinterpret_cast<const GainsArgs*>((const void*)__builtin_amdgcn_kernarg_segment_ptr());
    const double dt = g.s.kp.dt, two_wvel = g.s.kp.w_vel * 2, lamb = g.lamb;
    double* ko = g.k_out + (size_t)b * 2 * N;
    double* Ko = g.K_out + (size_t)b * 8 * N;
    Value V;
    Rec c;
    Gains gn;
    int j = N - 1;
    bool ok = true;
    for (; j >= 0; --j) {
      const double* r = rec + (size_t)j * REC_W;
      c.lx0 = r[0]; c.lx1 = r[1]; c.lx2 = r[2]; c.l00 = r[3]; c.l01 = r[4]; c.l11 = r[5];
      c.lu0 = r[6]; c.lu1 = r[7]; c.luu0 = r[8]; c.luu1 = r[9];
      c.al = r[10]; c.be = r[11]; c.ga = r[12]; c.de = r[13]; c.p = r[14]; c.q = r[15];
      if (j == N - 1) value_terminal(V, c, two_wvel);  // I/iLQR.cpp:108-113
      riccati_step<false>(c, V, dt, two_wvel, lamb, gn, ok);
      if (!ok) break;
      double* kj = ko + 2 * (size_t)j;
      double* Kj = Ko + 8 * (size_t)j;
      kj[0] = gn.g[0]; kj[1] = gn.g[1];
      // K[8t + r + 2c]: column-major 2×4, from {K00..K03, K10..K13}
      Kj[0] = gn.g[2]; Kj[1] = gn.g[6]; Kj[2] = gn.g[3]; Kj[3] = gn.g[7];
      Kj[4] = gn.g[4]; Kj[5] = gn.g[8]; Kj[6] = gn.g[5]; Kj[7] = gn.g[9];
    }
    for (; j >= 0; --j) {  // (a failed step: zero from there down)
      ko[2 * (size_t)j] = 0.0; ko[2 * (size_t)j + 1] = 0.0;
      for (int i = 0; i < 8; ++i) Ko[8 * (size_t)j + i] = 0.0;
    }
    if (g.ok_out) g.ok_out[b] = ok ? 1 : 0;
  }
}

}  // namespace

size_t gains_lds_bytes(int N, int n_path_samples) {
  return ((size_t)2 * n_path_samples + (size_t)2 * (N + 1) + (size_t)REC_W * N) * sizeof(double);
}

hipError_t launch_gains(const GainsArgs& a, hipStream_t stream) {
  if (a.s.B <= 0) return hipSuccess;
  const size_t lds = gains_lds_bytes(a.s.N, a.s.kp.n_samples);
  if (a.s.n_samples > 0) hipLaunchKernelGGL(cilqr_gains_kernel<true>, dim3(a.s.B), dim3(WAVE), lds, stream, a);
  else hipLaunchKernelGGL(cilqr_gains_kernel<false>, dim3(a.s.B), dim3(WAVE), lds, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
