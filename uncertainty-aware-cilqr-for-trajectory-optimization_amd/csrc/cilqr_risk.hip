// cilqr_risk.hip — collision risk of S closed-loop rollouts per solve WITHOUT storing a rollout (cilqr_rollout_risk*, include/cilqr.h):
// the rollout of cilqr_rollout.hip and, at every state it passes, the obstacle constraints c = 1 - d'Pd of cilqr_score.hip, reduced on
// the way to what a risk-bounded pick needs — which rows hit, the worst c and where and when it occurs, the hits per step.
//
// Nothing here is a floating-point sum.  Hit counts are integers; (max c, lowest row, lowest entry) is lexicographic.  Both come out
// the same in any evaluation order, so the mapping is free: lane = rollout row (the rollout kernel's), not the score kernel's 256
// lanes per row with their fixed summation tree.
//
// Mapping: a workgroup is 64·min(4, ceil(S/64)) lanes of ONE solve; solve b has G = ceil(S/256) workgroups, the grid is B·G.  Per
// workgroup, once, into LDS: the nominal records {X_t(4), U_t + k_scale·k_t (2), K_t(8)} by load_nominal, as in cilqr_rollout_kernel;
// the solve's obstacle entries, made by obs_entry_at through the strides of cilqr_obstacles — the call the score kernel makes, so
// the entries carry the same bits — stored [t][m] so that a step's M entries are consecutive; N per-step hit counters.  In the
// step loop every lane reads the same LDS address (a broadcast) and keeps its state in registers.
// u_t, the state and c are formed by the definitions of cilqr_rollout_core.hpp, which cilqr_rollout.hip and cilqr_score.hip use too:
// WORST_C is bit-equal to the worst SCORE_MAX_C of the stored-rows path.
// A wavefront whose share of S is partial computes its idle lanes on a zero offset and counts nothing for them; a wavefront with no
// row at all skips the loop.  Every row index is formed in 64 bits.  A solve's results depend on its own inputs and offsets alone.
// Arguments are read through kernel_args (the phase_args manner of cilqr_device.hpp): no scratch memory, no spilled register, 128
// vector registers at most (make check).
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

__device__ __forceinline__ const RolloutRiskArgs& risk_args() { return kernel_args<RolloutRiskArgs>(); }

// One partial record (a workgroup's) or G of them → the outputs of solve b.  Run by ONE wavefront.  Record g is
// {hit rows, worst c, its row, its entry} at rec + g*stride (doubles) with its N int32 step counts at counts + 2*g*stride: the
// partials buffer for G > 1, the workgroup's own LDS for G = 1 — the same statements either way.
__device__ __forceinline__ void risk_finish(const RolloutRiskArgs& a, int b, int G, int lane, const double* rec, const int32_t* counts,
                                            long long stride) {
  const int N = a.s.N, S = a.S;
  int32_t* step_hits = a.step_hits ? a.step_hits + (long long)b * N : nullptr;
  int most = 0, first = NO_INDEX;
  for (int t = lane; t < N; t += WAVE) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += counts[2 * g * stride + t];
    if (step_hits) step_hits[t] = n;
    most = max(most, n);
    if (n > 0) first = min(first, t);
  }
  for (int o = 32; o > 0; o >>= 1) {
    most = max(most, __shfl_xor(most, o, WAVE));
    first = min(first, __shfl_xor(first, o, WAVE));
  }
  if (lane == 0) {
    long long hit_rows = 0;
    double max_c = -__builtin_huge_val();
    int max_r = NO_INDEX, max_e = NO_INDEX;
    for (int g = 0; g < G; ++g) {  // ascending: lower rows first
      const double* p = rec + g * stride;
      hit_rows += (long long)p[0];
      row_merge(max_c, max_r, max_e, p[1], (int)p[2], (int)p[3]);
    }
    const double share = (double)hit_rows / (double)S;
    double* out = a.risk + (long long)b * CILQR_ROLLOUT_RISK_FIELDS;
    out[CILQR_RR_COLLISION] = share;
    out[CILQR_RR_WORST_C] = max_c;
    out[CILQR_RR_WORST_ROW] = max_e == NO_INDEX ? -1.0 : (double)max_r;
    out[CILQR_RR_WORST_ENTRY] = max_e == NO_INDEX ? -1.0 : (double)max_e;
    out[CILQR_RR_FIRST_STEP] = first == NO_INDEX ? -1.0 : (double)first;
    out[CILQR_RR_STEP_SHARE] = (double)most / (double)S;
    if (a.total) a.total[b] = gated_total(a.base[b], share, a.max_risk);
  }
}

// LDS (dynamic): [nominal: N·NOM_W + 4 (X_N)][entries: N·M·ENT_W][worst c per wavefront: 4][the workgroup's record: 4] | int32:
// [step counters: N][row, entry, hit rows per wavefront: 3·4]
__global__ __launch_bounds__(RISK_THREADS) void cilqr_rollout_risk_kernel(RolloutRiskArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE, threads = blockDim.x;
  const int N = a.s.N, M = a.s.M, S = a.S, G = a.G;
  const int b = blockIdx.x / G, s0 = (blockIdx.x - b * G) * RISK_THREADS;
  const int n_rows = min(threads, S - s0);  // rows of this workgroup
  const bool active = tid < n_rows;
  double* nom = lds;
  double* ent = nom + (size_t)N * NOM_W + 4;
  double* red_c = ent + (size_t)N * M * ENT_W;
  double* rec = red_c + RISK_WAVES;
  int* cnt = reinterpret_cast<int*>(rec + 4);
  int* red_r = cnt + N;
  int* red_e = red_r + RISK_WAVES;
  int* red_h = red_e + RISK_WAVES;

  load_nominal(risk_args(), b, N, tid, threads, nom, cnt);  // (and the step counters cleared)
  // ---- the obstacle entries of solve b → LDS, [t][m]
  {
    const SolveArgs& s = phase_args();  // (RolloutRiskArgs starts with its SolveArgs)
    const int n_ent = M * N;
    for (int e = tid; e < n_ent; e += threads) {
      const int m = e / N, t = e - m * N;
      const ObsEntry en = obs_entry_at(s.kp, s, b, m, t);
      double* w = ent + ((size_t)t * M + m) * ENT_W;
      w[0] = en.ox; w[1] = en.oy; w[2] = en.co; w[3] = en.so; w[4] = en.ia2; w[5] = en.ib2;
    }
  }
  __syncthreads();

  double max_c = -__builtin_huge_val();
  int max_e = NO_INDEX;
  bool hit_any = false;
  if (wave * WAVE < n_rows) {  // (wavefront-uniform: a wavefront without a row has nothing to do)
    State st = start_state(risk_args(), nom, b, s0 + tid, active);
    const KParams& kp = phase_params();
    for (int t = 0; t < N; ++t) {
      double u0, u1;
      feedback_control(st, nom + (size_t)t * NOM_W, u0, u1);
      bool hit = state_lost(st, u0, u1);
      {
#pragma clang fp contract(off)  // the sign of c decides a hit
        const ObsConsts oc = make_obs_consts(kp, st.x, st.y, st.c, st.s);
        const double* w = ent + (size_t)t * M * ENT_W;
        for (int m = 0; m < M; ++m, w += ENT_W) {
          const ObsEntry en{w[0], w[1], w[2], w[3], w[4], w[5]};
          double cf, cr;
          circle_constraints(oc, en, cf, cr);
          cmax_merge(max_c, max_e, fmax(cf, cr), m * N + t);
          hit = hit || cf > 0.0 || cr > 0.0;
        }
      }
      hit = hit && active;
      hit_any = hit_any || hit;
      const unsigned long long hitting = __ballot(hit);
      if (lane == 0 && hitting) atomicAdd(&cnt[t], __popcll(hitting));
      st = dyn_step(kp, st, u0, u1);
    }
  }

  // ---- reduction: butterflies inside the wavefronts, then the wavefronts in order by one lane
  int max_r = active && max_e != NO_INDEX ? s0 + tid : NO_INDEX;
  if (max_r == NO_INDEX) { max_c = -__builtin_huge_val(); max_e = NO_INDEX; }
  wave_row_merge(max_c, max_r, max_e);
  const int wave_hits = __popcll(__ballot(hit_any));
  if (lane == 0) { red_c[wave] = max_c; red_r[wave] = max_r; red_e[wave] = max_e; red_h[wave] = wave_hits; }
  __syncthreads();  // (every counter is final)
  if (tid == 0) {
    int hit_rows = wave_hits;
    const int waves = threads / WAVE;
    for (int w = 1; w < waves; ++w) {
      row_merge(max_c, max_r, max_e, red_c[w], red_r[w], red_e[w]);
      hit_rows += red_h[w];
    }
    rec[0] = (double)hit_rows; rec[1] = max_c; rec[2] = (double)max_r; rec[3] = (double)max_e;
  }
  __syncthreads();
  const RolloutRiskArgs& q = risk_args();
  if (G == 1) {  // one record per solve: the first wavefront writes the outputs itself, from LDS, by the finish kernel's statements
    if (wave == 0) risk_finish(q, b, 1, lane, rec, cnt, 0);
    return;
  }
  double* part = q.partials + (long long)blockIdx.x * q.part_stride;
  int32_t* pc = reinterpret_cast<int32_t*>(part + RISK_PART_DOUBLES);
  for (int t = tid; t < N; t += threads) pc[t] = cnt[t];
  if (tid < 4) part[tid] = rec[tid];
}

// G > 1: one wavefront per solve joins its G partial records in ascending order.
__global__ __launch_bounds__(WAVE) void cilqr_rollout_risk_finish_kernel(RolloutRiskArgs a) {
  const RolloutRiskArgs& q = risk_args();
  const int b = blockIdx.x, G = q.G;
  const double* part = q.partials + (long long)b * G * q.part_stride;
  risk_finish(q, b, G, threadIdx.x, part, reinterpret_cast<const int32_t*>(part + RISK_PART_DOUBLES), q.part_stride);
}

}  // namespace

size_t rollout_risk_lds_bytes(int N, int M) {
  return ((size_t)N * NOM_W + 4 + (size_t)N * M * ENT_W + RISK_WAVES + 4) * sizeof(double) + ((size_t)N + 3 * RISK_WAVES) * sizeof(int32_t);
}

hipError_t launch_rollout_risk(const RolloutRiskArgs& a, hipStream_t stream) {
  return launch_risk_pair(cilqr_rollout_risk_kernel, cilqr_rollout_risk_finish_kernel, a, a.s.B, a.S, a.G, rollout_risk_lds_bytes(a.s.N, a.s.M),
                          stream);
}

}  // namespace cilqr
