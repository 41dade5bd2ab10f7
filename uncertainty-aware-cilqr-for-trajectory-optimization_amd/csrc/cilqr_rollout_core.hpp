// cilqr_rollout_core.hpp — the closed-loop rollout step and the reductions around it, ONE definition each for the kernels that
// run it (cilqr_rollout.hip stores the rows; cilqr_risk.hip, cilqr_risk_sampled.hip and cilqr_risk_map.hip reduce them on the way)
// and for the kernels that share its merges and gates (cilqr_score.hip, cilqr_chance.hip, cilqr_chance_map.hip, cilqr_tighten.hip,
// cilqr_map_probes.hpp).  Per row, with x'_0 = X_0 + delta:
//   u_t = (U_t + k_scale·k_t) + K_t (x'_t − X_t)   (iLQR::forward_pass, I/iLQR.cpp:68-86; unclamped, the heading difference not wrapped)
//   x'_{t+1} = Model::forward_simulate(x'_t, u_t)   (dyn_step: the clamps act on a copy)
// The bit-equalities the tests assert — fused WORST_C == stored-rows SCORE_MAX_C, sampled == materialised, WORST_OCC == the map
// cost's own lookup — hold because every kernel forms these values by the statements below; where a kernel writes one of them out
// (its registers or its measured time were worse through the call) a comment there names the definition here as its twin.
#pragma once

#include "cilqr_device.hpp"

namespace cilqr {
namespace dev {

constexpr int NOM_W = 14;  // doubles per step of the nominal copy in LDS: {X_t(4), U_t + k_scale·k_t (2), K_t(8)}
constexpr int ENT_W = 6;   // doubles per obstacle entry (ObsEntry)
constexpr int NO_INDEX = 0x7fffffff;

// The kernel's whole argument block through a pointer the compiler cannot trace back to the preloaded arguments (as phase_args of
// cilqr_device.hpp): what a phase reads through it is loaded there, not carried through every phase.
template <class A>
__device__ __forceinline__ const A& kernel_args() {
  const A* q = reinterpret_cast<const A*>((const void*)__builtin_amdgcn_kernarg_segment_ptr());
  asm volatile("" : "+s"(q));
  return *q;
}

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < 1.7e308; }  // no library call (NaN fails every comparison)

// What a risk-bounded pick ranks by: the base cost, or NaN where it is not finite or the share exceeds the bound.
__device__ __forceinline__ double gated_total(double base, double share, double max_risk) {
  return is_finite(base) && !(share > max_risk) ? base : __builtin_nan("");
}

// (max value, lowest index): lexicographic, as amin_merge of cilqr_select.hip with the order of the value reversed; a NaN never wins
__device__ __forceinline__ void cmax_merge(double& c0, int& e0, double c1, int e1) {
  if (c1 > c0 || (c1 == c0 && e1 < e0)) { c0 = c1; e0 = e1; }
}
// (max value, lowest row) with the row's own lowest entry carried along
__device__ __forceinline__ void row_merge(double& c0, int& r0, int& e0, double c1, int r1, int e1) {
  if (c1 > c0 || (c1 == c0 && r1 < r0)) { c0 = c1; r0 = r1; e0 = e1; }
}
// row_merge over the 64 lanes by xor butterflies: every lane ends with the wavefront's triple
__device__ __forceinline__ void wave_row_merge(double& c, int& r, int& e) {
  for (int o = 32; o > 0; o >>= 1) {
    const double oc = __shfl_xor(c, o, WAVE);
    const int orow = __shfl_xor(r, o, WAVE);
    const int oe = __shfl_xor(e, o, WAVE);
    row_merge(c, r, e, oc, orow, oe);
  }
}
__device__ __forceinline__ int wave_sum_int(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// c = 1 - d'Pd of both ego circles (I/Obstacle.cpp:65-73, 86-94): the statements of obs_prep, which keeps q2·c only
__device__ __forceinline__ void circle_constraints(const ObsConsts& k, const ObsEntry& e, double& cf, double& cr) {
#pragma clang fp contract(off)
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const double ex = (side == 0 ? k.fxp : k.rxp) - e.ox, ey = (side == 0 ? k.fyp : k.ryp) - e.oy;
    const double d0 = __builtin_fma(e.co, ex, e.so * ey);
    const double d1 = __builtin_fma(e.co, ey, -(e.so * ex));
    const double c = 1 - __builtin_fma(d0 * e.ia2, d0, (d1 * e.ib2) * d1);
    if (side == 0) cf = c; else cr = c;
  }
}

// The nominal trajectory and gains of solve b → nom: NOM_W doubles per step, then X_N.  `q`: any block with X, U, k, K, k_scale;
// `zero`: null, or N per-step counters cleared in the same pass.  The caller's barrier follows.
template <class Q>
__device__ __forceinline__ void load_nominal(const Q& q, int b, int N, int tid, int threads, double* nom, int* zero = nullptr) {
  const double* X = q.X + (size_t)b * 4 * (N + 1);
  const double* U = q.U + (size_t)b * 2 * N;
  const double* k = q.k + (size_t)b * 2 * N;
  const double* K = q.K + (size_t)b * 8 * N;
  const double ks = q.k_scale;
  for (int t = tid; t < N; t += threads) {
    double* r = nom + (size_t)t * NOM_W;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = X[4 * t + i];
    r[4] = U[2 * t] + ks * k[2 * t];
    r[5] = U[2 * t + 1] + ks * k[2 * t + 1];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[6 + i] = K[8 * (size_t)t + i];
    if (zero) zero[t] = 0;
  }
  if (tid < 4) nom[(size_t)N * NOM_W + tid] = X[4 * N + tid];
}

// Row `row` of solve b at step 0: X_0 + its offset (64-bit indices); a lane that is not `active` starts on a zero offset.
template <class Q>
__device__ __forceinline__ State start_state(const Q& q, const double* nom, int b, int row, bool active) {
  double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
  if (active) {
    const double* d = q.delta + (long long)b * q.delta_bs + 4 * (long long)row;
    d0 = d[0]; d1 = d[1]; d2 = d[2]; d3 = d[3];
  }
  State st;
  st.x = nom[0] + d0; st.y = nom[1] + d1; st.v = nom[2] + d2; st.th = nom[3] + d3;
  sincos_fast(st.th, &st.s, &st.c);
  return st;
}

// u_t from the step's nominal record r.  K[r + 2c]: the dot product over c = 0..3, then (U + k_scale·k) + it, as
// oracle_forward_pass sums.
__device__ __forceinline__ void feedback_control(const State& st, const double* r, double& u0, double& u1) {
  const double e0 = st.x - r[0], e1 = st.y - r[1], e2 = st.v - r[2], e3 = st.th - r[3];
  const double f0 = fma(r[12], e3, fma(r[10], e2, fma(r[8], e1, r[6] * e0)));
  const double f1 = fma(r[13], e3, fma(r[11], e2, fma(r[9], e1, r[7] * e0)));
  u0 = r[4] + f0; u1 = r[5] + f1;
}

// A row whose state or control is no longer finite counts as hitting from that step on.
__device__ __forceinline__ bool state_lost(const State& st, double u0, double u1) {
  return !(is_finite(st.x) && is_finite(st.y) && is_finite(st.v) && is_finite(st.th) && is_finite(u0) && is_finite(u1));
}

}  // namespace dev

// The launch the fused risk kernels share: `main_kernel` on B·G workgroups of 64·min(4, ceil(S/64)) lanes, then, for G > 1,
// `finish_kernel` on B wavefronts.
template <class A>
hipError_t launch_risk_pair(void (*main_kernel)(A), void (*finish_kernel)(A), const A& a, int B, int S, int G, size_t lds_bytes,
                            hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int waves = (S + dev::WAVE - 1) / dev::WAVE;
  const int threads = dev::WAVE * (waves < RISK_WAVES ? waves : RISK_WAVES);
  const long long blocks = (long long)B * G;
  hipLaunchKernelGGL(main_kernel, dim3((unsigned)blocks), dim3(threads), lds_bytes, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || G == 1) return e;
  hipLaunchKernelGGL(finish_kernel, dim3(B), dim3(dev::WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
