// cilqr_score.hip — scores solved trajectories (cilqr_score_batch*, include/cilqr.h): per solve the tracking cost of
// Constraints::get_J, the VALUES of the control and obstacle barriers the solve only differentiates, the uncertainty-map cost,
// the worst obstacle constraint c = 1 - d'Pd and where it occurs, the worst control constraint and the collision share.  One
// pass over what a solve kernel evaluates in every linearisation; run after the solve, in front of the min-cost pick.
//
// Mapping: one workgroup of SCORE_THREADS lanes per solve, whatever the batch.  The score of a solve is a function of that
// solve's inputs alone, bit for bit: every partial result lives in a fixed lane (step t and entry e = m*N + t belong to lane
// index mod SCORE_THREADS), lanes are joined by xor butterflies (both partners form the same commutative sum) and the four
// wavefronts' results by one lane in wavefront order — a reduction tree that depends on (N, M) alone.
//   phase 0  lanes over the S path samples → LDS (sample_xy: the samples every solve kernel sees)
//   phase 1  lanes over the steps t < N, three loops so that each keeps its own constants in scalar registers: cos/sin of the ego
//            heading → LDS, closest path sample by a full strict-< scan (I/Constraints.cpp:43-56), stage cost; the four control
//            barriers (I/Constraints.cpp:110-131); the map cost (unc_cost_add).  Their wavefront sums go to LDS before phase 2.
//   phase 2  lanes over the entries e < M*N: make_obs_entry (strided table, or nominal pose + sample offset by plain additions),
//            c on both ego circles, the two barrier values, running (max c, lowest e); sampled obstacles count, per (t, o), the
//            samples with c > 0 on either circle in LDS integers (integer adds: any order gives the same count)
// Every phase reads its arguments through phase_args / phase_params (cilqr_device.hpp): no scratch memory, no spilled register,
// 128 vector registers at most (make check).
// cilqr_score_rollouts launches the same kernel over B·S rows, `rows` = S of them per solve (instantiation ROWS; S = 1 launches the
// score calls' own instantiation): row r is scored against solve r / S; cilqr_risk_kernel then reduces each solve's rows (one
// wavefront per solve, the same butterflies).
// x_N carries no cost, as in the reference (get_state_cost and get_J visit t < N).
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int SCORE_WAVES = SCORE_THREADS / WAVE;
constexpr int RED_SLOTS = 8;  // doubles per wavefront in the cross-wavefront stage

// (the epilogue's pointers and thresholds are loaded there, not carried through every phase)
__device__ __forceinline__ const ScoreArgs& score_args() { return kernel_args<ScoreArgs>(); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, WAVE);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
  return v;
}

// Entry (m, t) of solve b and its weight.  SAMPLED: m = o*n_samples + s is nominal obstacle o moved by sample s's offset — the
// pose the materialised call is given, formed by the same plain additions, through the same make_obs_entry.
template <bool SAMPLED>
__device__ __forceinline__ ObsEntry score_entry(const SolveArgs& a, const double* wts, int b, int m, int t, int& o, double& w) {
  if (SAMPLED) {
    o = m / a.n_samples;
    const long long e = ((long long)b * a.M + o) * a.N + t;
    const double* np = a.obs_pose + 4 * e;
    const double* off = a.samp_off + 3 * (((long long)b * a.M + o) * a.n_samples + (m - o * a.n_samples));
    const double pose[4] = {np[0] + off[0], np[1] + off[1], np[2], np[3] + off[2]};
    w = a.samp_w;
    return make_obs_entry(a.kp, pose, a.obs_dim + 2 * e);
  }
  o = m;
  w = wts ? wts[m] : a.kp.w_obstacle;
  return obs_entry_at(a.kp, a, b, m, t);
}

// a.s: the solve's argument block (X_out = the trajectories to score; for SAMPLED, M = nominal obstacles); LDS (dynamic):
// [sx S][sy S][cos N][sin N][RED_SLOTS per wavefront][entry index per wavefront][n_obs*N counters]
struct LdsPath {  // the path samples as closest_sample reads them
  const double* sx;
  const double* sy;
  __device__ __forceinline__ void operator()(int s, double& x, double& y) const { x = sx[s]; y = sy[s]; }
};

// ROWS (cilqr_score_rollouts with more than one row per solve; never SAMPLED): row b is scored against solve b / rows, and the
// closest path sample is found by closest_sample's window — built to return the full scan's index, ties included (cilqr_device.hpp;
// its squared distances come from the shared helper, so only two samples equidistant to the last bit could be ordered differently),
// hence the same bits — because the scan over all samples on N of 256 lanes is most of a workgroup's time and there are B·S workgroups.
template <bool SAMPLED, bool ROWS = false>
__global__ __launch_bounds__(SCORE_THREADS) void cilqr_score_kernel(ScoreArgs a) {
  extern __shared__ double lds[];
  // (every phase reads the argument block through phase_args: its scalar registers are live for that phase only)
  // b: the row scored (X, U, the outputs); sb: the solve whose path, obstacles, weights and map it is scored against (rows == 1: b)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int sb = ROWS ? b / a.rows : b;
  const int N = a.s.N, S = a.s.kp.n_samples;
  double* sx = lds;
  double* sy = sx + S;
  double* ect = sy + S;
  double* est = ect + N;
  double* red = est + N;
  int* red_e = reinterpret_cast<int*>(red + SCORE_WAVES * RED_SLOTS);
  int* hits = red_e + SCORE_WAVES;  // SAMPLED only
  const double* X = a.s.X_out + (size_t)b * 4 * (N + 1);
  const int n_hits = SAMPLED ? a.s.M * N : 0;

  // ---- phase 0: the path samples; the collision counters
  {
    const SolveArgs& s = phase_args();
    const double* pc = s.poly + (size_t)sb * CILQR_POLY_COEFFS;
    SampleGrid g;
    make_sample_grid(g, s.xplan_fl[2 * (size_t)sb], s.xplan_fl[2 * (size_t)sb + 1], S);
    for (int i = tid; i < S; i += SCORE_THREADS) sample_xy(g, pc, i, sx[i], sy[i]);
    for (int i = tid; i < n_hits; i += SCORE_THREADS) hits[i] = 0;
  }
  __syncthreads();

  // ---- phase 1: the steps
  double track = 0.0, ctrl = 0.0, unc = 0.0, max_ctrl = -__builtin_huge_val();
  {
#pragma clang fp contract(off)  // the closest-point comparison decides an index
    const KParams& kp = phase_params();
    const double* U = phase_args().U + (size_t)b * 2 * N;
    SampleGrid grid;
    if (ROWS) make_sample_grid(grid, phase_args().xplan_fl[2 * (size_t)sb], phase_args().xplan_fl[2 * (size_t)sb + 1], S);
    for (int t = tid; t < N; t += SCORE_THREADS) {
      const double px = X[4 * t], py = X[4 * t + 1], v = X[4 * t + 2];
      const double u0 = U[2 * t], u1 = U[2 * t + 1];
      double ct, st;
      sincos_fast(X[4 * t + 3], &st, &ct);
      ect[t] = ct;
      est[t] = st;
      // I/Constraints.cpp:43-56: strict-< first minimum over all S samples
      int best = 0;
      if (ROWS) {
        best = closest_sample<false>(S, grid, px, py, LdsPath{sx, sy});
      } else {
        double md = (sx[0] - px) * (sx[0] - px) + (sy[0] - py) * (sy[0] - py);
        for (int i = 1; i < S; ++i) {
          const double d = (sx[i] - px) * (sx[i] - px) + (sy[i] - py) * (sy[i] - py);
          if (d < md) { md = d; best = i; }
        }
      }
      track = track + stage_cost(kp, px - sx[best], py - sy[best], v - kp.desired_speed, u0, u1);
    }
  }
  {
#pragma clang fp contract(off)
    // I/Constraints.cpp:110-131: the four control constraints and their barrier values q1·exp(q2·c); a loop of its own, which
    // keeps the scalar registers of its constants apart from the scan's
    const KParams& kp = phase_params();
    const double* U = phase_args().U + (size_t)b * 2 * N;
    for (int t = tid; t < N; t += SCORE_THREADS) {
      const double v = X[4 * t + 2], u0 = U[2 * t], u1 = U[2 * t + 1];
      const double c1 = u0 - kp.acc_max, c2 = kp.acc_min - u0;
      const double c3 = u1 - v * kp.yaw_hi, c4 = v * kp.yaw_lo - u1;
      max_ctrl = fmax(fmax(max_ctrl, fmax(c1, c2)), fmax(c3, c4));
      const double va = kp.q1_acc * exp_fast(kp.q2_acc * c1) + kp.q1_acc * exp_fast(kp.q2_acc * c2);
      const double vy = kp.q1_yawrate * exp_fast(kp.q2_yawrate * c3) + kp.q1_yawrate * exp_fast(kp.q2_yawrate * c4);
      ctrl = ctrl + (va + vy);
    }
  }
  // the map cost in a loop of its own, as in the solve kernels: its registers stay out of the other phases' allocation
  if (phase_args().unc.layer) {
    const UncArgs& u = phase_args().unc;
    const UncPose po = unc_pose(u, sb);
    for (int t = tid; t < N; t += SCORE_THREADS) {
      double g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0;  // (the derivatives are the solve's business)
      unc = unc + unc_cost_add(u, po, sb, X[4 * t], X[4 * t + 1], ect[t], est[t], g0, g1, h0, h1, h2);
    }
  }
  // (their wavefront sums leave the registers before phase 2: butterflies, then lane 0 → this wavefront's slots)
  track = wave_sum(track);
  ctrl = wave_sum(ctrl);
  unc = wave_sum(unc);
  max_ctrl = wave_max(max_ctrl);
  if (lane == 0) {
    double* r = red + wave * RED_SLOTS;
    r[0] = track; r[1] = ctrl; r[3] = unc; r[5] = max_ctrl;
  }
  __syncthreads();

  // ---- phase 2: the obstacle entries e = m*N + t
  double obst = 0.0, max_c = -__builtin_huge_val();
  int max_e = NO_INDEX;
  {
#pragma clang fp contract(off)  // the sign of c decides the collision share
    const SolveArgs& s = phase_args();
    const KParams& kp = s.kp;
    const double* Xb = s.X_out + (size_t)b * 4 * (N + 1);
    const int M = SAMPLED ? s.M * s.n_samples : s.M;
    const int n_ent = M * N;
    const double* wts = SAMPLED ? nullptr : obs_weights(s, sb);
    for (int e = tid; e < n_ent; e += SCORE_THREADS) {
      const int m = e / N, t = e - m * N;
      int o;
      double w;
      const ObsEntry en = score_entry<SAMPLED>(s, wts, sb, m, t, o, w);
      const ObsConsts oc = make_obs_consts(kp, Xb[4 * t], Xb[4 * t + 1], ect[t], est[t]);
      double cf, cr;
      circle_constraints(oc, en, cf, cr);
      const double val = kp.q1_front * exp_full(kp.q2_front * cf) + kp.q1_rear * exp_full(kp.q2_rear * cr);  // (any obstacle, however far)
      obst = obst + w * val;
      cmax_merge(max_c, max_e, fmax(cf, cr), e);
      if (SAMPLED && (cf > 0.0 || cr > 0.0)) atomicAdd(&hits[o * N + t], 1);
    }
  }

  // ---- reduction: butterflies inside the wavefronts, then wavefront 0 … SCORE_WAVES-1 in order
  obst = wave_sum(obst);
  for (int o = 32; o > 0; o >>= 1) {
    const double oc = __shfl_xor(max_c, o, WAVE);
    const int oe = __shfl_xor(max_e, o, WAVE);
    cmax_merge(max_c, max_e, oc, oe);
  }
  int worst = 0;  // SAMPLED: the largest counter
  __syncthreads();  // (every counter is final)
  for (int i = tid; i < n_hits; i += SCORE_THREADS) worst = max(worst, hits[i]);
  for (int o = 32; o > 0; o >>= 1) worst = max(worst, __shfl_xor(worst, o, WAVE));
  if (lane == 0) {
    double* r = red + wave * RED_SLOTS;
    r[2] = obst; r[4] = max_c; r[6] = (double)worst;
    red_e[wave] = max_e;
  }
  __syncthreads();
  if (tid == 0) {
#pragma clang fp contract(off)
    const ScoreArgs& fa = score_args();
    track = red[0]; ctrl = red[1]; unc = red[3]; max_ctrl = red[5];
    for (int w = 1; w < SCORE_WAVES; ++w) {
      const double* r = red + w * RED_SLOTS;
      track = track + r[0]; ctrl = ctrl + r[1]; obst = obst + r[2]; unc = unc + r[3];
      cmax_merge(max_c, max_e, r[4], red_e[w]);
      max_ctrl = fmax(max_ctrl, r[5]);
      worst = max(worst, (int)r[6]);
    }
    unc = unc * fa.w_uncertainty;
    const double collision = SAMPLED ? (double)worst / (double)fa.s.n_samples : (max_c > 0.0 ? 1.0 : 0.0);
    double* out = fa.score + (size_t)b * CILQR_SCORE_FIELDS;
    out[CILQR_SCORE_TRACK] = track;
    out[CILQR_SCORE_CONTROL] = ctrl;
    out[CILQR_SCORE_OBSTACLE] = obst;
    out[CILQR_SCORE_UNCERTAINTY] = unc;
    out[CILQR_SCORE_MAX_C] = max_c;
    out[CILQR_SCORE_MAX_C_ENTRY] = max_e == NO_INDEX ? -1.0 : (double)max_e;
    out[CILQR_SCORE_MAX_CTRL] = max_ctrl;
    out[CILQR_SCORE_COLLISION] = collision;
    if (fa.total) {
      const bool finite = is_finite(track) && is_finite(ctrl) && is_finite(obst) && is_finite(unc);
      const double sum = ((track + ctrl) + obst) + unc;
      fa.total[b] = finite && !(collision > fa.max_collision) ? sum : __builtin_nan("");
    }
  }
}

// Each solve's S score rows → its risk fields (cilqr_risk_field) and the `total` the pick ranks by.  One wavefront per solve: lane
// l takes rows l, l + 64, … in ascending order, the lanes are joined by the xor butterflies above — a tree fixed by S alone; the
// hit count is an integer, (worst c, lowest row) lexicographic.
__global__ __launch_bounds__(WAVE) void cilqr_risk_kernel(RiskArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x, S = a.S;
  const double* rows = a.row_score + (size_t)b * (size_t)S * CILQR_SCORE_FIELDS;
  double sum = 0.0, max_c = -__builtin_huge_val();
  int max_r = NO_INDEX, hits = 0;
  for (int r = lane; r < S; r += WAVE) {
    const double* q = rows + (size_t)r * CILQR_SCORE_FIELDS;
    const double track = q[CILQR_SCORE_TRACK], ctrl = q[CILQR_SCORE_CONTROL], obst = q[CILQR_SCORE_OBSTACLE], unc = q[CILQR_SCORE_UNCERTAINTY];
    const double c = q[CILQR_SCORE_MAX_C];
    const bool finite = is_finite(track) && is_finite(ctrl) && is_finite(obst) && is_finite(unc);
    hits += (c > 0.0 || !finite) ? 1 : 0;
    cmax_merge(max_c, max_r, c, r);
    sum = sum + (((track + ctrl) + obst) + unc);
  }
  sum = wave_sum(sum);
  for (int o = 32; o > 0; o >>= 1) {
    hits += __shfl_xor(hits, o, WAVE);
    const double oc = __shfl_xor(max_c, o, WAVE);
    const int orow = __shfl_xor(max_r, o, WAVE);
    cmax_merge(max_c, max_r, oc, orow);
  }
  if (lane == 0) {
    const double share = (double)hits / (double)S, mean = sum / (double)S;
    double* out = a.risk + (size_t)b * CILQR_RISK_FIELDS;
    out[CILQR_RISK_COLLISION] = share;
    out[CILQR_RISK_WORST_C] = max_c;
    out[CILQR_RISK_WORST_ROW] = max_r == NO_INDEX ? -1.0 : (double)max_r;
    out[CILQR_RISK_MEAN_TOTAL] = mean;
    if (a.total) a.total[b] = gated_total(mean, share, a.max_risk);
  }
}

}  // namespace

size_t score_lds_bytes(int N, int S, int n_counters) {
  return ((size_t)2 * S + (size_t)2 * N + (size_t)SCORE_WAVES * RED_SLOTS) * sizeof(double) +
         ((size_t)SCORE_WAVES + (size_t)n_counters) * sizeof(int);
}

hipError_t launch_score(const ScoreArgs& a, hipStream_t stream) {
  const SolveArgs& s = a.s;
  if (s.B <= 0) return hipSuccess;
  const bool sampled = s.n_samples > 0;
  const size_t lds = score_lds_bytes(s.N, s.kp.n_samples, sampled ? s.M * s.N : 0);
  if (sampled) hipLaunchKernelGGL(cilqr_score_kernel<true>, dim3(s.B), dim3(SCORE_THREADS), lds, stream, a);
  else if (a.rows > 1) hipLaunchKernelGGL((cilqr_score_kernel<false, true>), dim3(s.B), dim3(SCORE_THREADS), lds, stream, a);
  else hipLaunchKernelGGL(cilqr_score_kernel<false>, dim3(s.B), dim3(SCORE_THREADS), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_risk(const RiskArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(cilqr_risk_kernel, dim3(a.B), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
