// cilqr_chance_sampled.hip — analytic chance risk against sampled obstacles in compact form (cilqr_chance_risk_sampled*,
// include/cilqr.h): n_obs nominal trajectories, n_samples pose offsets each.  Σ_t is an INPUT (sigma_out of cilqr_chance_risk), so
// the N·n_obs·n_samples entries of a solve depend on nothing but X_t, six entries of Σ_t and the entry itself: there is no chain.
// Per entry the chance value p of cilqr_chance.hip (circle_chance_arg, cilqr_chance_entry.hpp) on the pose the materialised call
// would be given — the plain additions of score_entry<true> (cilqr_score.hip) through make_obs_entry, so p carries the bits of
// cilqr_chance_risk's entry_p on the materialised table; per (obstacle, step) the mean of its samples' p and the count of samples
// in nominal contact; per step the sum of the means over the obstacles.
//
// Mapping (the one of cilqr_chance_map.hip): wavefront = step t, a workgroup of CHANCE_SAMPLED_WAVES wavefronts takes as many
// consecutive steps of ONE solve, solve b has G = ceil(N / CHANCE_SAMPLED_WAVES) workgroups, the grid is B·G.  What depends on the
// step alone — the two circle centres, their levers, the six entries of Σ_t — is formed once per wavefront; centres and levers are
// moved to scalar registers (uniform_double).  Two loops over the step's entries, as in cilqr_chance.hip: the first forms every
// entry's erfc argument and leaves it in LDS, the second takes erfc and sums.  One loop holding both — or both inside a loop
// over chunks of entries — keeps the constants of the library sincos and of erfc live side by side: 157 to 167 vector registers
// against 103 this way.  LDS (dynamic): 8 bytes per entry and wavefront, 32·n_obs·n_samples bytes per workgroup whatever N is.
//
// Lanes and the sum over the samples.  W = the power of two with n_samples <= W, at least 2 and at most 64.  A wavefront is cut
// into 64/W segments of W lanes; pass i gives segment g the obstacle o = i·(64/W) + g, and lane j' of the segment takes its samples
// j = j', j' + W, ... (more than one only where n_samples > 64), adding their p in ascending j.  The W lane sums of a segment —
// +0 where a lane has no sample — meet in an xor butterfly over the offsets W/2 ... 1: a tree fixed by n_samples alone, the same
// for every obstacle, step and solve.  q(o, t) = that sum / n_samples; the count of samples in contact goes the same way as an
// integer.  r_t adds the q(o, t) in ascending o.
//
// Per step lane 0 writes one record {r_t, max_o q, max_m p, their o and m, the largest count} to the handle's step records (and r_t
// to the caller's step_risk); the finish kernel, one wavefront per solve, reduces the records over t: lane sums over t ascending and
// a butterfly (a tree fixed by N), lexicographic maxima.  No atomics anywhere.
// No scratch memory, no spilled register, 128 vector registers at most (make check).
#include "cilqr_chance_entry.hpp"
#include "cilqr_map_probes.hpp"

namespace cilqr {

using namespace dev;

namespace {

__device__ __forceinline__ const ChanceSampledArgs& crs_args() { return const_kernel_args<ChanceSampledArgs>(); }

// What a step leaves for the finish kernel (CHANCE_SAMPLED_REC doubles).
struct StepRec {
  double r, q, p;   // r_t; the largest q(o, t) and the largest p(m, t) of the step (-inf where every one is NaN)
  int32_t o, m, n;  // their obstacle and materialised obstacle, lowest on equal values (NO_INDEX: none); the largest contact count
  int32_t pad;
};
static_assert(sizeof(StepRec) == CHANCE_SAMPLED_REC * sizeof(double), "step record size");

__global__ __launch_bounds__(CHANCE_SAMPLED_THREADS) void cilqr_chance_risk_sampled_kernel(ChanceSampledArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int N = a.s.N, G = a.G, n_obs = a.s.M, ns = a.s.n_samples;
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int t = g * CHANCE_SAMPLED_WAVES + wave;  // (wavefront-uniform)
  extern __shared__ double zbuf[];  // [CHANCE_SAMPLED_WAVES][n_obs·n_samples]: the step's erfc arguments between the two loops
  if (t >= N) return;  // (a workgroup's last wavefronts idle where N is no multiple of CHANCE_SAMPLED_WAVES; no barrier follows)

  // ---- what depends on the step alone
  const double* X = a.X + ((size_t)b * (N + 1) + t) * 4;
  const double* S = a.sigma + ((size_t)b * (N + 1) + t) * 16;
  const double x = X[0], y = X[1], th = X[3];
  double S6[6] = {S[0], S[4], S[12], S[5], S[13], S[15]};  // xx, xy, xθ, yy, yθ, θθ: (r, c) at [r + 4c], row <= column
  // (Σ_t is pinned in vector registers: beside the centres and levers, and the constants of the entry's library sincos, its
  // twelve scalar registers are the ones that would be spilled)
#pragma unroll
  for (int i = 0; i < 6; ++i) CILQR_PIN(S6[i]);
  double sn, cs;
  sincos_fast(th, &sn, &cs);
  const ObsConsts oc = make_obs_consts(crs_args().s.kp, x, y, cs, sn);
  const double lf = crs_args().s.kp.ego_front, lr = -crs_args().s.kp.ego_rear;
  const double fx = uniform_double(oc.fxp), fy = uniform_double(oc.fyp), rx = uniform_double(oc.rxp), ry = uniform_double(oc.ryp);
  const double lfx = uniform_double(-lf * sn), lfy = uniform_double(lf * cs), lrx = uniform_double(-lr * sn), lry = uniform_double(lr * cs);
  ObsConsts ou = {};  // (circle_constraints reads the four centres only)
  ou.fxp = fx; ou.fyp = fy; ou.rxp = rx; ou.ryp = ry;

  // ---- segments of W lanes: the pass from o0 gives segment g the obstacle o0 + g and its lane j' the samples j', j' + W, ...
  int W = 2;
  while (W < ns && W < WAVE) W <<= 1;
  const int per = WAVE / W, seg = lane / W, jl = lane & (W - 1);
  const int E = n_obs * ns;
  double* zb = zbuf + (size_t)wave * E;  // (a lane reads back what it wrote itself: no barrier)
  int max_n = 0;
  // -- the entries' arguments → LDS, and the contact counts
  for (int o0 = 0; o0 < n_obs; o0 += per) {
    const int o = o0 + seg;
    int hits = 0;
    for (int j0 = 0; j0 < ns; j0 += W) {  // (one round unless n_samples > 64)
      const int j = j0 + jl;
      if (o < n_obs && j < ns) {
        const ChanceSampledArgs& z = crs_args();
        // the materialised pose by the plain additions of score_entry<true> (cilqr_score.hip)
        const long long e = ((long long)b * n_obs + o) * N + t;
        const double* np = z.s.obs_pose + 4 * e;
        const double* off = z.s.samp_off + 3 * (((long long)b * n_obs + o) * ns + j);
        const double pose[4] = {np[0] + off[0], np[1] + off[1], np[2], np[3] + off[2]};
        const ObsEntry en = make_obs_entry(z.s.kp, pose, z.s.obs_dim + 2 * e);
        // erfc decreases: the larger of the two circles' chance values is the one of the smaller argument (a NaN never wins)
        const double zf = circle_chance_arg<true>(en, fx, fy, lfx, lfy, S6);
        const double zr = circle_chance_arg<false>(en, rx, ry, lrx, lry, S6);
        zb[o * ns + j] = fmin(zf, zr);
        double cf, cr;
        circle_constraints(ou, en, cf, cr);
        hits += cf > 0.0 || cr > 0.0 ? 1 : 0;
      }
    }
    for (int w = W >> 1; w > 0; w >>= 1) hits += __shfl_xor(hits, w, WAVE);  // (inside the segment: W is a power of two)
    max_n = max(max_n, hits);  // (a segment without an obstacle counts 0)
  }
  // -- erfc in a loop of its own (side by side with the entry's arithmetic it needs more than 128 registers), and the sums
  double r_sum = 0.0, max_q = -__builtin_huge_val(), max_p = -__builtin_huge_val();
  int at_q = NO_INDEX, at_p = NO_INDEX;
  for (int o0 = 0; o0 < n_obs; o0 += per) {
    const int o = o0 + seg;
    double acc = 0.0;
    for (int j0 = 0; j0 < ns; j0 += W) {  // (ascending j within the lane)
      const int j = j0 + jl;
      if (o < n_obs && j < ns) {
        const int m = o * ns + j;
        const double p = 0.5 * erfc(zb[m]);
        if (crs_args().entry_p) crs_args().entry_p[((size_t)b * E + m) * N + t] = p;
        cmax_merge(max_p, at_p, p, m);
        acc += p;
      }
    }
    for (int w = W >> 1; w > 0; w >>= 1) acc += __shfl_xor(acc, w, WAVE);  // (a lane without a sample adds +0)
    const double q = acc / (double)ns;
    if (o < n_obs) {
      cmax_merge(max_q, at_q, q, o);
      if (jl == 0 && crs_args().pair_p) crs_args().pair_p[((size_t)b * n_obs + o) * N + t] = q;
    }
    const int n_seg = min(per, n_obs - o0);
    for (int sg = 0; sg < n_seg; ++sg) r_sum += __shfl(q, sg * W, WAVE);  // ascending o; every lane forms the same sum
  }
  for (int w = 32; w > 0; w >>= 1) {
    const double oq = __shfl_xor(max_q, w, WAVE), op = __shfl_xor(max_p, w, WAVE);
    const int iq = __shfl_xor(at_q, w, WAVE), ip = __shfl_xor(at_p, w, WAVE);
    cmax_merge(max_q, at_q, oq, iq);
    cmax_merge(max_p, at_p, op, ip);
    max_n = max(max_n, __shfl_xor(max_n, w, WAVE));
  }
  if (lane == 0) {
    const ChanceSampledArgs& z = crs_args();
    // a lost step (read anew: carried across the two loops the mark would be spilled)
    const double* Xt = z.X + ((size_t)b * (N + 1) + t) * 4;
    const double* St = z.sigma + ((size_t)b * (N + 1) + t) * 16;
    const bool lost = !(is_finite(Xt[0]) && is_finite(Xt[1]) && is_finite(Xt[3]) && is_finite(St[0]) && is_finite(St[4]) &&
                        is_finite(St[12]) && is_finite(St[5]) && is_finite(St[13]) && is_finite(St[15]));
    const double r = lost ? 1.0 : fmin(1.0, r_sum);  // (fmin: a sum that is NaN gives 1)
    const size_t at = (size_t)b * N + t;
    StepRec rec;
    rec.r = r; rec.q = max_q; rec.p = max_p; rec.o = at_q; rec.m = at_p; rec.n = max_n; rec.pad = 0;
    ((StepRec*)z.steps)[at] = rec;
    if (z.step_risk) z.step_risk[at] = r;
  }
}

// One wavefront per solve: the N step records → risk [CILQR_CRS_FIELDS] and total.
__global__ __launch_bounds__(WAVE) void cilqr_chance_risk_sampled_finish_kernel(ChanceSampledArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, N = a.s.N;
  const StepRec* recs = (const StepRec*)a.steps + (size_t)b * N;
  double max_r = -__builtin_huge_val(), max_q = -__builtin_huge_val(), max_p = -__builtin_huge_val(), sum = 0.0;
  int at_r = NO_INDEX, at_q = NO_INDEX, at_p = NO_INDEX, max_n = 0;
  for (int t = lane; t < N; t += WAVE) {  // ascending t within the lane
    const StepRec rec = recs[t];
    cmax_merge(max_r, at_r, rec.r, t);
    sum += rec.r;
    if (rec.o != NO_INDEX) cmax_merge(max_q, at_q, rec.q, rec.o * N + t);
    if (rec.m != NO_INDEX) cmax_merge(max_p, at_p, rec.p, rec.m * N + t);
    max_n = max(max_n, rec.n);
  }
  for (int w = 32; w > 0; w >>= 1) {
    const double orr = __shfl_xor(max_r, w, WAVE), oq = __shfl_xor(max_q, w, WAVE), op = __shfl_xor(max_p, w, WAVE);
    const int ir = __shfl_xor(at_r, w, WAVE), iq = __shfl_xor(at_q, w, WAVE), ip = __shfl_xor(at_p, w, WAVE);
    cmax_merge(max_r, at_r, orr, ir);
    cmax_merge(max_q, at_q, oq, iq);
    cmax_merge(max_p, at_p, op, ip);
    max_n = max(max_n, __shfl_xor(max_n, w, WAVE));
    sum += __shfl_xor(sum, w, WAVE);
  }
  if (lane == 0) {
    const double sum_risk = fmin(1.0, sum);
    double* out = a.risk + (size_t)b * CILQR_CRS_FIELDS;
    out[CILQR_CRS_STEP_RISK] = max_r;
    out[CILQR_CRS_WORST_STEP] = (double)at_r;
    out[CILQR_CRS_SUM_RISK] = sum_risk;
    out[CILQR_CRS_MAX_PAIR_P] = at_q == NO_INDEX ? 0.0 : max_q;
    out[CILQR_CRS_MAX_PAIR] = at_q == NO_INDEX ? -1.0 : (double)at_q;
    out[CILQR_CRS_MAX_ENTRY_P] = at_p == NO_INDEX ? 0.0 : max_p;
    out[CILQR_CRS_MAX_ENTRY] = at_p == NO_INDEX ? -1.0 : (double)at_p;
    out[CILQR_CRS_NOMINAL_SHARE] = (double)max_n / (double)a.s.n_samples;
    if (a.total) {
      const double bounded = (a.flags & CILQR_CHANCE_SAMPLED_BOUND_SUM) ? sum_risk : max_r;
      a.total[b] = gated_total(a.base[b], bounded, a.max_risk);
    }
  }
}

}  // namespace

size_t chance_risk_sampled_lds_bytes(int n_obs, int n_samples) {
  return (size_t)CHANCE_SAMPLED_WAVES * (size_t)n_obs * (size_t)n_samples * sizeof(double);
}

hipError_t launch_chance_risk_sampled(const ChanceSampledArgs& a, hipStream_t stream) {
  if (a.s.B <= 0 || a.s.N <= 0) return hipSuccess;
  const long long blocks = (long long)a.s.B * a.G;
  hipLaunchKernelGGL(cilqr_chance_risk_sampled_kernel, dim3((unsigned)blocks), dim3(CHANCE_SAMPLED_THREADS),
                     chance_risk_sampled_lds_bytes(a.s.M, a.s.n_samples), stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_chance_risk_sampled_finish_kernel, dim3(a.s.B), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
