// cilqr_risk.hip — collision risk of S closed-loop rollouts per solve WITHOUT storing a rollout (cilqr_rollout_risk*, include/cilqr.h):
// the rollout of cilqr_rollout.hip and, at every state it passes, the obstacle constraints c = 1 - d'Pd of cilqr_score.hip, reduced on
// the way to what a risk-bounded pick needs — which rows hit, the worst c and where and when it occurs, the hits per step.
//
// Nothing here is a floating-point sum.  Hit counts are integers; (max c, lowest row, lowest entry) is lexicographic.  Both come out
// the same in any evaluation order, so the mapping is free: lane = rollout row (the rollout kernel's), not the score kernel's 256
// lanes per row with their fixed summation tree.
//
// Mapping: a workgroup is 64·min(4, ceil(S/64)) lanes of ONE solve; solve b has G = ceil(S/256) workgroups, the grid is B·G.  Per
// workgroup, once, into LDS: the nominal records {X_t(4), U_t + k_scale·k_t (2), K_t(8)} exactly as cilqr_rollout_kernel forms them;
// the solve's obstacle entries, made by obs_entry_at through the strides of cilqr_obstacles — the call the score kernel makes, so
// the entries carry the same bits — stored [t][m] so that a step's M entries are consecutive; N per-step hit counters.  In the
// step loop every lane reads the same LDS address (a broadcast) and keeps its state in registers.
// u_t, the state and c are formed by the statements of cilqr_rollout.hip and cilqr_score.hip (circle_constraints and cmax_merge are
// restated verbatim): WORST_C is bit-equal to the worst SCORE_MAX_C of the stored-rows path.
// A wavefront whose share of S is partial computes its idle lanes on a zero offset and counts nothing for them; a wavefront with no
// row at all skips the loop.  Every row index is formed in 64 bits.  A solve's results depend on its own inputs and offsets alone.
// Arguments are read through risk_args (the phase_args manner of cilqr_device.hpp): no scratch memory, no spilled register, 128
// vector registers at most (make check).
#include "cilqr_device.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int NOM_W = 14;    // doubles per step of the nominal copy (cilqr_rollout.hip)
constexpr int ENT_W = 6;     // doubles per obstacle entry (ObsEntry)
constexpr int NO_INDEX = 0x7fffffff;

__device__ __forceinline__ const RolloutRiskArgs& risk_args() {
  const RolloutRiskArgs* q = reinterpret_cast<const RolloutRiskArgs*>((const void*)__builtin_amdgcn_kernarg_segment_ptr());
  asm volatile("" : "+s"(q));
  return *q;
}

// (max c, lowest entry): cilqr_score.hip, verbatim
__device__ __forceinline__ void cmax_merge(double& c0, int& e0, double c1, int e1) {
  if (c1 > c0 || (c1 == c0 && e1 < e0)) { c0 = c1; e0 = e1; }
}
// (max c, lowest row) with the row's own lowest entry carried along
__device__ __forceinline__ void row_merge(double& c0, int& r0, int& e0, double c1, int r1, int e1) {
  if (c1 > c0 || (c1 == c0 && r1 < r0)) { c0 = c1; r0 = r1; e0 = e1; }
}

// c = 1 - d'Pd of both ego circles (I/Obstacle.cpp:65-73, 86-94): cilqr_score.hip, verbatim
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
    if (a.total) {
      const double base = a.base[b];
      a.total[b] = fabs(base) < 1.7e308 && !(share > a.max_risk) ? base : __builtin_nan("");
    }
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

  // ---- the nominal trajectory and gains of solve b → LDS (the statements of cilqr_rollout_kernel); the counters
  {
    const RolloutRiskArgs& q = risk_args();
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
      cnt[t] = 0;
    }
    if (tid < 4) nom[(size_t)N * NOM_W + tid] = X[4 * N + tid];
  }
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
    // ---- this lane's start
    State st;
    {
      const RolloutRiskArgs& q = risk_args();
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
      if (active) {
        const double* d = q.delta + (long long)b * q.delta_bs + 4 * (long long)(s0 + tid);
        d0 = d[0]; d1 = d[1]; d2 = d[2]; d3 = d[3];
      }
      st.x = nom[0] + d0; st.y = nom[1] + d1; st.v = nom[2] + d2; st.th = nom[3] + d3;
      sincos_fast(st.th, &st.s, &st.c);
    }
    const KParams& kp = phase_params();
    const double big = 1.7e308;  // finite test without library calls (NaN fails every comparison)
    for (int t = 0; t < N; ++t) {
      const double* r = nom + (size_t)t * NOM_W;
      const double e0 = st.x - r[0], e1 = st.y - r[1], e2 = st.v - r[2], e3 = st.th - r[3];
      // K[r + 2c]: the dot product over c = 0..3, then (U + k_scale·k) + it (cilqr_rollout.hip)
      const double f0 = fma(r[12], e3, fma(r[10], e2, fma(r[8], e1, r[6] * e0)));
      const double f1 = fma(r[13], e3, fma(r[11], e2, fma(r[9], e1, r[7] * e0)));
      const double u0 = r[4] + f0, u1 = r[5] + f1;
      bool hit = !(fabs(st.x) < big && fabs(st.y) < big && fabs(st.v) < big && fabs(st.th) < big && fabs(u0) < big && fabs(u1) < big);
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
  for (int o = 32; o > 0; o >>= 1) {
    const double oc = __shfl_xor(max_c, o, WAVE);
    const int orow = __shfl_xor(max_r, o, WAVE);
    const int oe = __shfl_xor(max_e, o, WAVE);
    row_merge(max_c, max_r, max_e, oc, orow, oe);
  }
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
  if (a.s.B <= 0) return hipSuccess;
  const int waves = (a.S + WAVE - 1) / WAVE;
  const int threads = WAVE * (waves < RISK_WAVES ? waves : RISK_WAVES);
  const long long blocks = (long long)a.s.B * a.G;
  hipLaunchKernelGGL(cilqr_rollout_risk_kernel, dim3((unsigned)blocks), dim3(threads), rollout_risk_lds_bytes(a.s.N, a.s.M), stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.G == 1) return e;
  hipLaunchKernelGGL(cilqr_rollout_risk_finish_kernel, dim3(a.s.B), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
