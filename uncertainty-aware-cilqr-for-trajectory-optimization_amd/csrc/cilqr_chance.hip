// cilqr_chance.hip — analytic pose-noise risk of a solved plan (cilqr_chance_risk*, include/cilqr.h): ONE 4x4 covariance per solve
// carried through the linear closed loop x' - X_{t+1} = (A_t + B_t K_t)(x - X_t) that the gains define around the plan, and from
// Σ_t a Gaussian chance value per (obstacle, step, ego circle) — the probability that the solver's own constraint c = 1 - d'Pd is
// positive under N(c̄, g'Σ_t g).  No samples, no seed: the work of one rollout row in place of S of them.
//
// Mapping: one workgroup per solve, 64·min(4, ceil(max(N, M·N)/64)) lanes — a function of (N, M) alone, as is every summation
// order below, so a solve's bits do not depend on the batch.  Three phases:
//   stage    lane = step t (strided): X_t, U_t, K_t → F_t = A_t + B_t K_t, row-major, into LDS; the step's "lost" mark (an input
//            that is not finite) into the slot that later holds r_t.  The N sincos of the headings run side by side here, not on
//            the chain.
//   chain    the first wavefront alone.  Lane i < 10 owns one row <= column entry (r, c) of Σ and holds it in a register.  A step
//            moves the ten entries to scalar registers by v_readlane (20 of them: no LDS round trip on the serial path, and the
//            products then take Σ as a scalar operand), forms  Σ'_rc = Σ_k F_rk (Σ_l Σ_kl F_cl) + W_rc  from its two rows of F_t —
//            fetched from LDS one step ahead — and stores Σ_{t+1}[r][c] and its mirror to LDS without waiting for the store.
//            Lanes 10..63 repeat lane 9's arithmetic and store nothing: no divergence around the v_readlane.
//   entries  lane = obstacle entry e = m·N + t (strided): the entry by make_obs_entry through the strides of cilqr_obstacles and
//            the circle centres by make_obs_consts on sincos_fast of the heading — the score kernel's statements, so c̄ carries its
//            bits — then g, s = sqrt(g'Σ_t g) and z = -c̄/(s√2) per circle; p = erfc(min z)/2 = max of the two circles' → LDS, entry_p.
//   then     lane = step: r_t = min(1, Σ_m p[m, t]) in ascending m; and the first wavefront reduces: (max r_t, lowest t) and
//            (max p, lowest entry) lexicographically, Σ_t r_t by a strided partial per lane and a butterfly, the largest position
//            standard deviation in closed form.
// LDS (dynamic, doubles): [F: 16·N][Σ: 16·(N + 1)][r: N][p: M·N] = 8·(33·N + M·N + 16) bytes.
// No scratch memory, no spilled register (make check).
#include "cilqr_chance_entry.hpp"

namespace cilqr {

using namespace dev;

namespace {

__device__ __forceinline__ const ChanceArgs& chance_args() { return kernel_args<ChanceArgs>(); }

// The value lane `SRC` of the wavefront holds, in scalar registers.
template <int SRC>
__device__ __forceinline__ double lane_value(double v) {
  const unsigned long long w = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)w, SRC), hi = __builtin_amdgcn_readlane((unsigned)(w >> 32), SRC);
  return __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

// (circle_chance_arg = circle_chance_form + chance_arg, the entry's arithmetic: cilqr_chance_entry.hpp, shared with
// cilqr_chance_sampled.hip)

// COV: cilqr_chance_risk_cov — every entry's form gains the obstacle's covariance, read at the entry's own index; an entry whose
// three values are not all finite gets the argument of p = 1.  Nothing else differs, and COV = false is cilqr_chance_risk's kernel.
template <bool COV>
__global__ __launch_bounds__(CHANCE_THREADS) void cilqr_chance_risk_kernel(typename ChanceKernelArgs<COV>::type a) {
  extern __shared__ __attribute__((aligned(16))) double chance_lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int N = a.s.N, M = a.s.M, b = blockIdx.x;
  double* Fm = chance_lds;                    // [N][16], row-major
  double* sig = Fm + (size_t)16 * N;          // [N + 1][16], symmetric
  double* rt = sig + (size_t)16 * (N + 1);    // [N]
  double* pe = rt + N;                        // [M·N], entry m·N + t
  const double* X = a.X + (size_t)b * 4 * (N + 1);

  // ---- stage: F_t and the step's lost mark
  {
    const ChanceArgs& q = chance_args();
    const KParams& kp = phase_params();
    const double* U = q.U + (size_t)b * 2 * N;
    const double* K = q.K + (size_t)b * 8 * N;
    const double dt = kp.dt, h2 = kp.half_dt2;
    for (int t = tid; t < N; t += threads) {
      const double x = X[4 * t], y = X[4 * t + 1], v = X[4 * t + 2], th = X[4 * t + 3];
      const double u0 = U[2 * t], u1 = U[2 * t + 1];
      double k[8];
      bool ok = is_finite(x) && is_finite(y) && is_finite(v) && is_finite(th) && is_finite(u0) && is_finite(u1);
#pragma unroll
      for (int i = 0; i < 8; ++i) { k[i] = K[8 * (size_t)t + i]; ok = ok && is_finite(k[i]); }
      double sn, cs;
      sincos_fast(th, &sn, &cs);
      const double adv = v * dt + u0 * h2;
      const double a0[4] = {1.0, 0.0, dt * cs, -sn * adv}, a1[4] = {0.0, 1.0, dt * sn, cs * adv};
      const double b0 = h2 * cs, b1 = h2 * sn;
      double* f = Fm + (size_t)16 * t;
#pragma unroll
      for (int l = 0; l < 4; ++l) {  // K[r + 2c]: control r, state c
        f[l] = a0[l] + b0 * k[2 * l];
        f[4 + l] = a1[l] + b1 * k[2 * l];
        f[8 + l] = (l == 2 ? 1.0 : 0.0) + dt * k[2 * l];
        f[12 + l] = (l == 3 ? 1.0 : 0.0) + dt * k[2 * l + 1];
      }
      rt[t] = ok ? 0.0 : 1.0;
    }
  }
  __syncthreads();

  // ---- chain: Σ_0 → Σ_N on the first wavefront
  if (wave == 0) {
    const ChanceArgs& q = chance_args();
    const int i = lane < 9 ? lane : 9;  // entry (r, c), r <= c: 0:(0,0) 1:(0,1) 2:(0,2) 3:(0,3) 4:(1,1) 5:(1,2) 6:(1,3) 7:(2,2) 8:(2,3) 9:(3,3)
    const int r = i < 4 ? 0 : i < 7 ? 1 : i < 9 ? 2 : 3;
    const int c = i - (r == 0 ? 0 : r == 1 ? 3 : r == 2 ? 5 : 6);
    const bool owner = lane < 10;
    double s = q.sigma0[(long long)b * q.sigma0_bs + r + 4 * c];
    const double w = q.W ? q.W[r + 4 * c] : 0.0;
    if (owner) { sig[r + 4 * c] = s; sig[c + 4 * r] = s; }
    double fr[4], fc[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) { fr[l] = Fm[4 * r + l]; fc[l] = Fm[4 * c + l]; }
    for (int t = 0; t < N; ++t) {
      // the next step's rows leave LDS before this step's arithmetic (the last step re-reads its own: nothing past F is touched)
      const double* fn = Fm + (size_t)16 * (t + 1 < N ? t + 1 : t);
      double nr[4], nc[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) { nr[l] = fn[4 * r + l]; nc[l] = fn[4 * c + l]; }
      const double s00 = lane_value<0>(s), s01 = lane_value<1>(s), s02 = lane_value<2>(s), s03 = lane_value<3>(s);
      const double s11 = lane_value<4>(s), s12 = lane_value<5>(s), s13 = lane_value<6>(s);
      const double s22 = lane_value<7>(s), s23 = lane_value<8>(s), s33 = lane_value<9>(s);
      const double t0 = fma(s03, fc[3], fma(s02, fc[2], fma(s01, fc[1], s00 * fc[0])));
      const double t1 = fma(s13, fc[3], fma(s12, fc[2], fma(s11, fc[1], s01 * fc[0])));
      const double t2 = fma(s23, fc[3], fma(s22, fc[2], fma(s12, fc[1], s02 * fc[0])));
      const double t3 = fma(s33, fc[3], fma(s23, fc[2], fma(s13, fc[1], s03 * fc[0])));
      s = fma(fr[3], t3, fma(fr[2], t2, fma(fr[1], t1, fr[0] * t0))) + w;
      if (owner) {
        double* o = sig + (size_t)16 * (t + 1);
        o[r + 4 * c] = s;
        o[c + 4 * r] = s;
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) { fr[l] = nr[l]; fc[l] = nc[l]; }
    }
  }
  __syncthreads();

  // ---- Σ_t → sigma_out; the entries
  {
    const ChanceArgs& q = chance_args();
    if (q.sigma_out) {
      double* out = q.sigma_out + (size_t)b * 16 * (N + 1);
      for (int i = tid; i < 16 * (N + 1); i += threads) out[i] = sig[i];
    }
    const SolveArgs& s = phase_args();  // (ChanceArgs starts with its SolveArgs)
    const KParams& kp = phase_params();
    double* entry_p = q.entry_p ? q.entry_p + (size_t)b * M * N : nullptr;
    const int n_ent = M * N;
    for (int e = tid; e < n_ent; e += threads) {
      const int m = e / N, t = e - m * N;
      const ObsEntry en = obs_entry_at(kp, s, b, m, t);
      const double x = X[4 * t], y = X[4 * t + 1], th = X[4 * t + 3];
      double sn, cs;
      sincos_fast(th, &sn, &cs);
      const ObsConsts oc = make_obs_consts(kp, x, y, cs, sn);
      const double* S = sig + (size_t)16 * t;
      const double S6[6] = {S[0], S[4], S[12], S[5], S[13], S[15]};  // xx, xy, xθ, yy, yθ, θθ
      // erfc decreases: the larger of the two circles' chance values is the one of the smaller argument (a NaN never wins)
      const double lf = kp.ego_front, lr = -kp.ego_rear;
      if (COV) {
        const ChanceForm ff = circle_chance_form<true>(en, oc.fxp, oc.fyp, -lf * sn, lf * cs, S6);
        const ChanceForm fr = circle_chance_form<false>(en, oc.rxp, oc.ryp, -lr * sn, lr * cs, S6);
        // (the entry's index is formed again here, from a copy of e the compiler cannot trace: m, or the address, carried from the
        // entry's loads across the two forms takes the kernel past 128 registers)
        int ec = e;
        asm volatile("" : "+v"(ec));
        const int mc = ec / N, tc = ec - mc * N;
        const double* oc3 = kernel_args<ChanceCovArgs>().obs_cov + 3 * obs_entry_index(s, b, mc, tc);
        const double cxx = oc3[0], cxy = oc3[1], cyy = oc3[2];
        const double zf = chance_arg(ff.c, chance_form_with_cov(ff, cxx, cxy, cyy));
        const double zr = chance_arg(fr.c, chance_form_with_cov(fr, cxx, cxy, cyy));
        pe[e] = is_finite(cxx) && is_finite(cxy) && is_finite(cyy) ? fmin(zf, zr) : -__builtin_huge_val();
      } else {
        const double zf = circle_chance_arg<true>(en, oc.fxp, oc.fyp, -lf * sn, lf * cs, S6);
        const double zr = circle_chance_arg<false>(en, oc.rxp, oc.ryp, -lr * sn, lr * cs, S6);
        pe[e] = fmin(zf, zr);
      }
    }
    // (a loop of its own: erfc alone is live in it — side by side with the entry's arithmetic it needs more than 128 registers)
    for (int e = tid; e < n_ent; e += threads) {
      const double p = 0.5 * erfc(pe[e]);
      pe[e] = p;
      if (entry_p) entry_p[e] = p;
    }
  }
  __syncthreads();

  // ---- per step: Boole's bound over the obstacles, ascending m; a lost step, or one whose Σ_t is not finite, is 1
  {
    const ChanceArgs& q = chance_args();
    double* step_risk = q.step_risk ? q.step_risk + (size_t)b * N : nullptr;
    for (int t = tid; t < N; t += threads) {
      bool ok = rt[t] == 0.0;
      const double* S = sig + (size_t)16 * t;
#pragma unroll
      for (int i = 0; i < 16; ++i) ok = ok && is_finite(S[i]);
      double sum = 0.0;
      for (int m = 0; m < M; ++m) sum += pe[(size_t)m * N + t];
      const double v = ok ? fmin(1.0, sum) : 1.0;  // (fmin: a sum that is NaN gives 1)
      rt[t] = v;
      if (step_risk) step_risk[t] = v;
    }
  }
  __syncthreads();

  // ---- the fields, by the first wavefront
  if (wave != 0) return;
  double max_r = -__builtin_huge_val(), max_p = -__builtin_huge_val(), sum_r = 0.0, max_l = 0.0;
  int max_t = NO_INDEX, max_e = NO_INDEX;
  for (int t = lane; t < N; t += WAVE) {
    cmax_merge(max_r, max_t, rt[t], t);
    sum_r += rt[t];
  }
  for (int e = lane; e < M * N; e += WAVE) cmax_merge(max_p, max_e, pe[e], e);
  for (int t = lane; t <= N; t += WAVE) {
    const double* S = sig + (size_t)16 * t;
    const double hs = 0.5 * (S[0] + S[5]), hd = 0.5 * (S[0] - S[5]);
    max_l = fmax(max_l, hs + sqrt(hd * hd + S[4] * S[4]));  // λ_max of [[xx, xy], [xy, yy]]; a NaN never wins
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double orr = __shfl_xor(max_r, o, WAVE), op = __shfl_xor(max_p, o, WAVE);
    const int ot = __shfl_xor(max_t, o, WAVE), oe = __shfl_xor(max_e, o, WAVE);
    cmax_merge(max_r, max_t, orr, ot);
    cmax_merge(max_p, max_e, op, oe);
    sum_r += __shfl_xor(sum_r, o, WAVE);
    max_l = fmax(max_l, __shfl_xor(max_l, o, WAVE));
  }
  if (lane == 0) {
    const ChanceArgs& q = chance_args();
    const double step = max_t == NO_INDEX ? 0.0 : max_r, sum = fmin(1.0, sum_r);
    double* out = q.risk + (size_t)b * CILQR_CHANCE_FIELDS;
    out[CILQR_CR_STEP_RISK] = step;
    out[CILQR_CR_WORST_STEP] = M == 0 || max_t == NO_INDEX ? -1.0 : (double)max_t;
    out[CILQR_CR_SUM_RISK] = sum;
    out[CILQR_CR_MAX_P] = max_e == NO_INDEX ? 0.0 : max_p;
    out[CILQR_CR_MAX_ENTRY] = max_e == NO_INDEX ? -1.0 : (double)max_e;
    out[CILQR_CR_MAX_POS_SIGMA] = sqrt(max_l);
    if (q.total) {
      const double base = q.base[b];
      const double bounded = (q.flags & CILQR_CHANCE_BOUND_SUM) ? sum : step;
      q.total[b] = is_finite(base) && !(bounded > q.max_risk) ? base : __builtin_nan("");
    }
  }
}

}  // namespace

size_t chance_risk_lds_bytes(int N, int M) { return ((size_t)33 * N + (size_t)M * N + 16) * sizeof(double); }

namespace {
int chance_threads(int N, int M) {
  const long long work = (long long)N * (M > 1 ? M : 1);
  const long long waves = (work + WAVE - 1) / WAVE;
  return WAVE * (int)(waves < CHANCE_THREADS / WAVE ? waves : CHANCE_THREADS / WAVE);
}
}  // namespace

hipError_t launch_chance_risk(const ChanceArgs& a, hipStream_t stream) {
  if (a.s.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(cilqr_chance_risk_kernel<false>, dim3((unsigned)a.s.B), dim3(chance_threads(a.s.N, a.s.M)), chance_risk_lds_bytes(a.s.N, a.s.M),
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_chance_risk_cov(const ChanceCovArgs& a, hipStream_t stream) {
  if (a.s.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(cilqr_chance_risk_kernel<true>, dim3((unsigned)a.s.B), dim3(chance_threads(a.s.N, a.s.M)),
                     chance_risk_lds_bytes(a.s.N, a.s.M), stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
