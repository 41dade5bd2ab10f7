// cilqr_risk_sampled.hip — collision risk of S closed-loop rollouts per solve against SAMPLED obstacles, with no rollout stored and no
// materialised obstacle table (cilqr_rollout_risk_sampled*, include/cilqr.h): the rollout of cilqr_rollout.hip and, at every state
// it passes, the constraints c = 1 - d'Pd of cilqr_score.hip against the n_obs·n_samples pose samples of that step, reduced on the
// way to hit COUNTS h(r, t, o) — the samples of obstacle o that row r touches at step t — and the worst c.
//
// Nothing here is a floating-point sum: counts are integers, (max c, lowest row, lowest entry) is lexicographic.  Any evaluation
// order gives the same results, so the mapping is free: lane = rollout row, as in cilqr_risk.hip.
//
// Mapping: a workgroup is 64·min(4, ceil(S/64)) lanes of ONE solve; solve b has G = ceil(S/256) workgroups, the grid is B·G.  Per
// workgroup, once, into LDS: the nominal records {X_t(4), U_t + k_scale·k_t (2), K_t(8)} by load_nominal, as in
// cilqr_rollout_kernel; N per-step counters and N·n_obs per-(t, o) counters.  The materialised table (48·n_obs·n_samples·N bytes: 614 KB at 8 x 32
// samples and N = 50) cannot be resident, so each step's n_obs·n_samples entries are built COOPERATIVELY into a double-buffered
// step buffer: while every lane evaluates step t from one half by LDS broadcast reads, it builds its ceil(n_obs·n_samples / lanes)
// entries of step t + 1 into the other — the pose formed by the plain additions of score_entry<true> (cilqr_score.hip), through
// the same make_obs_entry, so that the entries carry the bits of the materialised table — with ONE barrier per step.  Every
// wavefront of a workgroup builds and meets the barriers, also one that has no row (cilqr_risk.hip lets such a wavefront skip its
// loop: there nothing is built inside it).
// u_t, the state and c are formed by the definitions of cilqr_rollout_core.hpp, as in cilqr_risk.hip: WORST_C is bit-equal to that
// of cilqr_rollout_risk on the materialised obstacles.
// Per step a wavefront adds its rows' max_o h to the step counter and, per obstacle, its rows' h to the (t, o) counter: a butterfly
// sum, then one LDS integer atomic by lane 0 (skipped when no row of the wavefront touches the obstacle).
// Arguments are read through kernel_args (the phase_args manner of cilqr_device.hpp): no scratch memory, no spilled register, 128
// vector registers at most (make check).
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

__device__ __forceinline__ const RolloutRiskArgs& risk_args() { return kernel_args<RolloutRiskArgs>(); }

// The n_obs·n_samples entries of step t of solve b → buf[m], m = o·n_samples + j: nominal obstacle o moved by sample j's offset, the
// pose the materialised call is given, formed by the same plain additions (score_entry<true>), in 64-bit indices.
__device__ __forceinline__ void build_step(const SolveArgs& s, int b, int t, int tid, int threads, double* buf) {
  const int n_obs = s.M, ns = s.n_samples, ME = n_obs * ns, N = s.N;
  for (int m = tid; m < ME; m += threads) {
    const int o = m / ns;
    const long long ob = (long long)b * n_obs + o;
    const long long e = ob * N + t;
    const double* np = s.obs_pose + 4 * e;
    const double* off = s.samp_off + 3 * (ob * ns + (m - o * ns));
    const double pose[4] = {np[0] + off[0], np[1] + off[1], np[2], np[3] + off[2]};
    const ObsEntry en = make_obs_entry(s.kp, pose, s.obs_dim + 2 * e);
    double* w = buf + (size_t)m * ENT_W;
    w[0] = en.ox; w[1] = en.oy; w[2] = en.co; w[3] = en.so; w[4] = en.ia2; w[5] = en.ib2;
  }
}

// One partial record (a workgroup's) or G of them → the outputs of solve b.  Run by ONE wavefront.  Record g is {sum over rows of
// max h, worst c, its row, its entry, rows with any hit} at rec + g*stride (doubles) with its int32 counters at counts + 2*g*stride —
// N step counts, then N·n_obs (t, o) counts: the partials workspace for G > 1, the workgroup's own LDS for G = 1 — the same
// statements either way.
__device__ __forceinline__ void risk_finish(const RolloutRiskArgs& a, int b, int G, int lane, const double* rec, const int32_t* counts,
                                            long long stride) {
  const int N = a.s.N, S = a.S, n_pairs = N * a.s.M;
  int32_t* step_hits = a.step_hits ? a.step_hits + (long long)b * N : nullptr;
  int most = 0, first = NO_INDEX, pair_most = 0;
  for (int t = lane; t < N; t += WAVE) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += counts[2 * g * stride + t];
    if (step_hits) step_hits[t] = n;
    most = max(most, n);
    if (n > 0) first = min(first, t);
  }
  for (int i = lane; i < n_pairs; i += WAVE) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += counts[2 * g * stride + N + i];
    pair_most = max(pair_most, n);
  }
  for (int o = 32; o > 0; o >>= 1) {
    most = max(most, __shfl_xor(most, o, WAVE));
    first = min(first, __shfl_xor(first, o, WAVE));
    pair_most = max(pair_most, __shfl_xor(pair_most, o, WAVE));
  }
  if (lane == 0) {
    long long sum_h = 0, any_rows = 0;
    double max_c = -__builtin_huge_val();
    int max_r = NO_INDEX, max_e = NO_INDEX;
    for (int g = 0; g < G; ++g) {  // ascending: lower rows first
      const double* p = rec + g * stride;
      sum_h += (long long)p[0];
      any_rows += (long long)p[4];
      row_merge(max_c, max_r, max_e, p[1], (int)p[2], (int)p[3]);
    }
    const double draws = (double)((long long)S * a.s.n_samples);
    const double share = (double)sum_h / draws;
    double* out = a.risk + (long long)b * CILQR_RRS_FIELDS;
    out[CILQR_RRS_COLLISION] = share;
    out[CILQR_RRS_WORST_C] = max_c;
    out[CILQR_RRS_WORST_ROW] = max_e == NO_INDEX ? -1.0 : (double)max_r;
    out[CILQR_RRS_WORST_ENTRY] = max_e == NO_INDEX ? -1.0 : (double)max_e;
    out[CILQR_RRS_FIRST_STEP] = first == NO_INDEX ? -1.0 : (double)first;
    out[CILQR_RRS_STEP_SHARE] = (double)most / draws;
    out[CILQR_RRS_ANY_SHARE] = (double)any_rows / (double)S;
    out[CILQR_RRS_PAIR_SHARE] = (double)pair_most / draws;
    if (a.total) a.total[b] = gated_total(a.base[b], share, a.max_risk);
  }
}

// LDS (dynamic): [nominal: N·NOM_W + 4 (X_N)][step buffer: 2 halves of n_obs·n_samples·ENT_W][worst c per wavefront: 4][the
// workgroup's record: 8] | int32: [step counters: N][(t, o) counters: N·n_obs][row, entry, sum of max h, hit rows per wavefront: 4·4]
__global__ __launch_bounds__(RISK_THREADS) void cilqr_rollout_risk_sampled_kernel(RolloutRiskArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE, threads = blockDim.x;
  const int N = a.s.N, n_obs = a.s.M, ns = a.s.n_samples, S = a.S, G = a.G;
  const int ME = n_obs * ns;
  const int b = blockIdx.x / G, s0 = (blockIdx.x - b * G) * RISK_THREADS;
  const int n_rows = min(threads, S - s0);  // rows of this workgroup
  const bool active = tid < n_rows;
  double* nom = lds;
  double* ent = nom + (size_t)N * NOM_W + 4;
  double* red_c = ent + (size_t)2 * ME * ENT_W;
  double* rec = red_c + RISK_WAVES;
  int* cnt = reinterpret_cast<int*>(rec + RISK_PART_DOUBLES);
  int* pair = cnt + N;
  int* red_r = pair + (size_t)N * n_obs;
  int* red_e = red_r + RISK_WAVES;
  int* red_s = red_e + RISK_WAVES;
  int* red_h = red_s + RISK_WAVES;

  load_nominal(risk_args(), b, N, tid, threads, nom);
  for (int i = tid; i < N * (1 + n_obs); i += threads) cnt[i] = 0;  // (cnt and pair are consecutive)
  // ---- the entries of step 0 → the first half of the step buffer
  build_step(phase_args(), b, 0, tid, threads, ent);  // (RolloutRiskArgs starts with its SolveArgs)
  __syncthreads();

  const bool has_rows = wave * WAVE < n_rows;  // (wavefront-uniform: a wavefront without a row builds and waits only)
  double max_c = -__builtin_huge_val();
  int max_e = NO_INDEX, row_h = 0;
  bool hit_any = false;
  State st = start_state(risk_args(), nom, b, s0 + tid, active);
  for (int t = 0; t < N; ++t) {
    // the entries of step t + 1 → the half nobody reads in this iteration
    if (t + 1 < N) build_step(phase_args(), b, t + 1, tid, threads, ent + (size_t)((t + 1) & 1) * ME * ENT_W);
    if (has_rows) {
      const KParams& kp = phase_params();
      const double* r = nom + (size_t)t * NOM_W;
      const double e0 = st.x - r[0], e1 = st.y - r[1], e2 = st.v - r[2], e3 = st.th - r[3];
      // (feedback_control and state_lost of cilqr_rollout_core.hpp, written out: through the calls the launch measured 1 % slower
      // at S = 1024, profiles/r16_rollout_core.txt)
      const double f0 = fma(r[12], e3, fma(r[10], e2, fma(r[8], e1, r[6] * e0)));
      const double f1 = fma(r[13], e3, fma(r[11], e2, fma(r[9], e1, r[7] * e0)));
      const double u0 = r[4] + f0, u1 = r[5] + f1;
      const bool lost = !(is_finite(st.x) && is_finite(st.y) && is_finite(st.v) && is_finite(st.th) && is_finite(u0) && is_finite(u1));
      int step_h = 0;  // max over o of h(r, t, o)
      {
#pragma clang fp contract(off)  // the sign of c decides a hit
        const ObsConsts oc = make_obs_consts(kp, st.x, st.y, st.c, st.s);
        const double* w = ent + (size_t)(t & 1) * ME * ENT_W;
        int m = 0;
        for (int o = 0; o < n_obs; ++o) {
          int h = 0;
          for (int j = 0; j < ns; ++j, ++m, w += ENT_W) {
            const ObsEntry en{w[0], w[1], w[2], w[3], w[4], w[5]};
            double cf, cr;
            circle_constraints(oc, en, cf, cr);
            cmax_merge(max_c, max_e, fmax(cf, cr), (int)((long long)m * N + t));
            h += (cf > 0.0 || cr > 0.0) ? 1 : 0;
          }
          h = active ? (lost ? ns : h) : 0;
          step_h = max(step_h, h);
          if (__ballot(h > 0)) {  // (wavefront-uniform)
            const int sum = wave_sum_int(h);
            if (lane == 0) atomicAdd(&pair[t * n_obs + o], sum);
          }
        }
      }
      row_h = max(row_h, step_h);
      hit_any = hit_any || step_h > 0;
      if (__ballot(step_h > 0)) {
        const int sum = wave_sum_int(step_h);
        if (lane == 0) atomicAdd(&cnt[t], sum);
      }
      st = dyn_step(kp, st, u0, u1);
    }
    __syncthreads();  // step t + 1 is built, and step t's half is free to be overwritten
  }

  // ---- reduction: butterflies inside the wavefronts, then the wavefronts in order by one lane
  int max_r = active && max_e != NO_INDEX ? s0 + tid : NO_INDEX;
  if (max_r == NO_INDEX) { max_c = -__builtin_huge_val(); max_e = NO_INDEX; }
  wave_row_merge(max_c, max_r, max_e);
  const int wave_h = wave_sum_int(row_h);
  const int wave_hits = __popcll(__ballot(hit_any));
  if (lane == 0) { red_c[wave] = max_c; red_r[wave] = max_r; red_e[wave] = max_e; red_s[wave] = wave_h; red_h[wave] = wave_hits; }
  __syncthreads();  // (every counter is final)
  if (tid == 0) {
    int sum_h = wave_h, hit_rows = wave_hits;
    const int waves = threads / WAVE;
    for (int w = 1; w < waves; ++w) {
      row_merge(max_c, max_r, max_e, red_c[w], red_r[w], red_e[w]);
      sum_h += red_s[w];
      hit_rows += red_h[w];
    }
    rec[0] = (double)sum_h; rec[1] = max_c; rec[2] = (double)max_r; rec[3] = (double)max_e; rec[4] = (double)hit_rows;
  }
  __syncthreads();
  const RolloutRiskArgs& q = risk_args();
  if (G == 1) {  // one record per solve: the first wavefront writes the outputs itself, from LDS, by the finish kernel's statements
    if (wave == 0) risk_finish(q, b, 1, lane, rec, cnt, 0);
    return;
  }
  double* part = q.partials + (long long)blockIdx.x * q.part_stride;
  int32_t* pc = reinterpret_cast<int32_t*>(part + RISK_PART_DOUBLES);
  for (int i = tid; i < N * (1 + n_obs); i += threads) pc[i] = cnt[i];
  if (tid < 5) part[tid] = rec[tid];
}

// G > 1: one wavefront per solve joins its G partial records in ascending order.
__global__ __launch_bounds__(WAVE) void cilqr_rollout_risk_sampled_finish_kernel(RolloutRiskArgs a) {
  const RolloutRiskArgs& q = risk_args();
  const int b = blockIdx.x, G = q.G;
  const double* part = q.partials + (long long)b * G * q.part_stride;
  risk_finish(q, b, G, threadIdx.x, part, reinterpret_cast<const int32_t*>(part + RISK_PART_DOUBLES), q.part_stride);
}

}  // namespace

size_t rollout_risk_sampled_lds_bytes(int N, int n_obs, int n_samples) {
  return ((size_t)N * NOM_W + 4 + (size_t)2 * n_obs * n_samples * ENT_W + RISK_WAVES + RISK_PART_DOUBLES) * sizeof(double) +
         ((size_t)N * (1 + n_obs) + 4 * RISK_WAVES) * sizeof(int32_t);
}

size_t rollout_risk_sampled_part_doubles(int N, int n_obs) {
  return RISK_PART_DOUBLES + ((size_t)N * (1 + n_obs) + 1) / 2;
}

hipError_t launch_rollout_risk_sampled(const RolloutRiskArgs& a, hipStream_t stream) {
  return launch_risk_pair(cilqr_rollout_risk_sampled_kernel, cilqr_rollout_risk_sampled_finish_kernel, a, a.s.B, a.S, a.G,
                          rollout_risk_sampled_lds_bytes(a.s.N, a.s.M, a.s.n_samples), stream);
}

}  // namespace cilqr
