// cilqr_risk_map.hip — map risk of S closed-loop rollouts per solve WITHOUT storing a rollout (cilqr_rollout_risk_map*,
// include/cilqr.h): the rollout of cilqr_rollout.hip and, at every state it passes, the probes_l × probes_w footprint probes and the
// bilinear lookup of the uncertainty map set on the handle (unc_cost_add, cilqr_device.hpp), reduced on the way to what a
// risk-bounded pick needs — which rows enter cells above an occupancy threshold, the worst occupancy touched and where and when,
// the hits per step, the rows that leave the known map.
//
// Nothing here is a floating-point sum.  Counts are integers; (max occupancy, lowest row, lowest entry) is lexicographic.  Both
// come out the same in any evaluation order, so the mapping is free and is the one of cilqr_risk.hip: lane = rollout row, a
// workgroup is 64·min(4, ceil(S/64)) lanes of ONE solve, solve b has G = ceil(S/256) workgroups, the grid is B·G.  Per workgroup,
// once, into LDS: the nominal records {X_t(4), U_t + k_scale·k_t (2), K_t(8)} by load_nominal, as in cilqr_rollout_kernel, and N
// per-step counters.  A counter holds the rows that hit at step t in its low 16 bits and the rows that are unknown at step t in
// its high 16 (a workgroup has at most 256 rows): one LDS atomic per wavefront and step feeds both from two ballot counts.
// u_t and the state are formed by the definitions of cilqr_rollout_core.hpp; probe positions, cell indices, the validity test and
// the interpolant are the statements of unc_cost_add, restated in cilqr_map_probes.hpp with contraction off, on the rollout state's
// own cos / sin (sincos_fast, carried by dyn_step): WORST_OCC is bit-equal to the occupancy the map cost interpolates at that probe.
//
// Load scheduling.  Nothing dyn_step needs comes from the map, so no lookup has to sit on the rollout's dependency chain.  The
// probes are taken in groups of PROBE_GROUP (probes_l, probes_w are runtime values): a group's addresses, validity of position and
// interpolation weights are computed first and its 4·PROBE_GROUP loads are issued together, unconditionally — a probe outside the
// map reads cells (0,0)..(1,1), which every accepted map has — and a group is consumed only after the NEXT group's loads are in
// flight.  The pipeline runs across the steps: the last group of step t is in flight while dyn_step advances the state (≈ 150 fp64
// instructions, sincos_fast among them), and the first group of step t + 1 leaves from the new state before that last group is
// used.  So between a load and its use lie a whole group's address arithmetic or the step itself, never nothing.  Two groups
// live at once cost vector registers: PROBE_GROUP = 3 — the node's 3 x 3 footprint in three groups, 12 loads each — is the
// largest that stays within 128 without a spill (profiles/r12_risk_map.txt lists the counts and times of 1, 2, 3 and 4).  The layer is read by GLOBAL loads (a flat load would also count against lgkmcnt, and every wait for
// an LDS record would wait for the layer) through the vector cache: the rows of a solve lie within a few cells of each other and i
// is contiguous, so a wavefront's gather falls into a handful of lines.  The map's constants and the dynamics' parameters come by
// SCALAR loads through a constant-address-space view of the argument block, read anew in every step: as vector loads (what a
// generic pointer gives once LDS stores are in the loop) each group began with a memory round trip of its own, and carried
// across the loop they do not fit the scalar registers.
// A wavefront whose share of S is partial computes its idle lanes on a zero offset and counts nothing for them; a wavefront with no
// row at all skips the loop.  Every row index is formed in 64 bits.  A solve's results depend on its own inputs and offsets alone.
// No scratch memory, no spilled vector or scalar register, 128 vector registers at most (make check).
#include "cilqr_map_probes.hpp"

namespace cilqr {

using namespace dev;

namespace {

// (the constant-address-space accessor, not kernel_args: why, at const_kernel_args in cilqr_map_probes.hpp)
__device__ __forceinline__ const MapRiskArgs& risk_args() { return const_kernel_args<MapRiskArgs>(); }

// One partial record (a workgroup's) or G of them → the outputs of solve b.  Run by ONE wavefront.  Record g is
// {hit rows, worst occupancy, its row, its entry, unknown rows} at rec + g*stride (doubles) with its N packed int32 step counters
// at counts + 2*g*stride: the partials buffer for G > 1, the workgroup's own LDS for G = 1 — the same statements either way.
__device__ __forceinline__ void map_risk_finish(const MapRiskArgs& a, int b, int G, int lane, const double* rec, const int32_t* counts,
                                                long long stride) {
  const int N = a.r.s.N, S = a.r.S;
  int32_t* step_hits = a.r.step_hits ? a.r.step_hits + (long long)b * N : nullptr;
  int32_t* unknown_hits = a.unknown_hits ? a.unknown_hits + (long long)b * N : nullptr;
  int most = 0, first = NO_INDEX;
  for (int t = lane; t < N; t += WAVE) {
    int n = 0, un = 0;
    for (int g = 0; g < G; ++g) {
      const int v = counts[2 * g * stride + t];
      n += v & 0xffff;
      un += v >> 16;
    }
    if (step_hits) step_hits[t] = n;
    if (unknown_hits) unknown_hits[t] = un;
    most = max(most, n);
    if (n > 0) first = min(first, t);
  }
  for (int o = 32; o > 0; o >>= 1) {
    most = max(most, __shfl_xor(most, o, WAVE));
    first = min(first, __shfl_xor(first, o, WAVE));
  }
  if (lane == 0) {
    long long hit_rows = 0, unknown_rows = 0;
    double max_o = -__builtin_huge_val();
    int max_r = NO_INDEX, max_e = NO_INDEX;
    for (int g = 0; g < G; ++g) {  // ascending: lower rows first
      const double* p = rec + g * stride;
      hit_rows += (long long)p[0];
      unknown_rows += (long long)p[4];
      row_merge(max_o, max_r, max_e, p[1], (int)p[2], (int)p[3]);
    }
    const double share = (double)hit_rows / (double)S;
    double* out = a.r.risk + (long long)b * CILQR_MAP_RISK_FIELDS;
    out[CILQR_MR_COLLISION] = share;
    out[CILQR_MR_WORST_OCC] = max_o;
    out[CILQR_MR_WORST_ROW] = max_e == NO_INDEX ? -1.0 : (double)max_r;
    out[CILQR_MR_WORST_ENTRY] = max_e == NO_INDEX ? -1.0 : (double)max_e;
    out[CILQR_MR_FIRST_STEP] = first == NO_INDEX ? -1.0 : (double)first;
    out[CILQR_MR_STEP_SHARE] = (double)most / (double)S;
    out[CILQR_MR_UNKNOWN] = (double)unknown_rows / (double)S;
    if (a.r.total) {
      const double base = a.r.base[b];
      a.r.total[b] = gated_total(base, share, a.r.max_risk);
    }
  }
}

// LDS (dynamic): [nominal: N·NOM_W + 4 (X_N)][worst occupancy per wavefront: 4][the workgroup's record: 8] | int32:
// [packed step counters: N][row, entry, hit rows, unknown rows per wavefront: 4·4]
struct Lds {
  double *nom, *red_o, *rec;
  int *cnt, *red_r, *red_e, *red_h, *red_u;
};
__device__ __forceinline__ Lds lds_layout(double* lds, int N) {
  Lds m;
  m.nom = lds;
  m.red_o = m.nom + (size_t)N * NOM_W + 4;
  m.rec = m.red_o + RISK_WAVES;
  m.cnt = reinterpret_cast<int*>(m.rec + RISK_PART_DOUBLES);
  m.red_r = m.cnt + N;
  m.red_e = m.red_r + RISK_WAVES;
  m.red_h = m.red_e + RISK_WAVES;
  m.red_u = m.red_h + RISK_WAVES;
  return m;
}
// The workgroup's place in the launch.  Formed from the argument block before the step loop and AGAIN after it: carried across
// the loop these scalars would be spilled.
struct Place {
  int N, G, b, s0, n_rows;
};
__device__ __forceinline__ Place place_of(int threads) {
  const MapRiskArgs& q = risk_args();
  Place w;
  w.N = q.r.s.N; w.G = q.r.G;
  w.b = blockIdx.x / w.G; w.s0 = (blockIdx.x - w.b * w.G) * RISK_THREADS;
  w.n_rows = min(threads, q.r.S - w.s0);  // rows of this workgroup
  return w;
}

__global__ __launch_bounds__(RISK_THREADS) void cilqr_rollout_risk_map_kernel(MapRiskArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);  // (scalar: the branch around the step loop saves no lane mask)
  const Place w = place_of(threads);
  const int N = w.N, b = w.b, s0 = w.s0, n_rows = w.n_rows;
  const bool active = tid < n_rows;
  const Lds m = lds_layout(lds, N);
  double* nom = m.nom;
  int* cnt = m.cnt;

  load_nominal(risk_args().r, b, N, tid, threads, nom, cnt);  // (and the step counters cleared)
  __syncthreads();

  double max_o = -__builtin_huge_val();
  int max_e = NO_INDEX;
  bool hit_any = false, unknown_any = false;
  if (wave * WAVE < n_rows) {  // (wavefront-uniform: a wavefront without a row has nothing to do)
    State st = start_state(risk_args().r, nom, b, s0 + tid, active);
    // (the map's constants and the dynamics' parameters are read anew, by scalar loads, where a step uses them: carried across the
    // loop they would not fit the scalar registers)
    UncPose po = unc_pose(risk_args().r.s.unc, b);
    po.px = uniform_double(po.px); po.py = uniform_double(po.py); po.cp = uniform_double(po.cp); po.sp = uniform_double(po.sp);
    const LayerPtr layer = (LayerPtr)(risk_args().r.s.unc.layer + (size_t)b * (size_t)risk_args().r.s.unc.stride);
    const int P = risk_args().r.s.unc.nl * risk_args().r.s.unc.nw;
    const double threshold = risk_args().occ_threshold;
    const bool unknown_hits = (risk_args().flags & CILQR_MAP_RISK_UNKNOWN_HITS) != 0;
    // the first group of step 0 leaves; from here on `cur` is a group whose loads are in flight
    int k = 0, l = 0;
    ProbeGroup cur;
    probes_issue(risk_args().r.s.unc, po, layer, st.x, st.y, st.c, st.s, is_finite(st.v), 0, k, l, cur);
    for (int t = 0; t < N; ++t) {
      bool hit = false, unknown = false;
      const UncArgs& u = risk_args().r.s.unc;
      for (int q0 = PROBE_GROUP; q0 < P; q0 += PROBE_GROUP) {  // the next group's loads leave before this group's are used
        ProbeGroup nx;
        probes_issue(u, po, layer, st.x, st.y, st.c, st.s, is_finite(st.v), q0, k, l, nx);
        probes_consume(cur, t, N, threshold, max_o, max_e, hit, unknown);
        cur = nx;
      }
      // the step's last group is in flight while the state advances
      double u0, u1;
      feedback_control(st, nom + (size_t)t * NOM_W, u0, u1);
      // (state_lost of cilqr_rollout_core.hpp, written out: through the call this kernel takes 132 vector registers, not 114)
      const bool lost = !(is_finite(st.x) && is_finite(st.y) && is_finite(st.v) && is_finite(st.th) && is_finite(u0) && is_finite(u1));
      st = dyn_step(risk_args().r.s.kp, st, u0, u1);
      // ... and the first group of the next step leaves before the last of this one is used
      ProbeGroup nx = {};
      k = 0; l = 0;
      if (t + 1 < N) probes_issue(risk_args().r.s.unc, po, layer, st.x, st.y, st.c, st.s, is_finite(st.v), 0, k, l, nx);
      probes_consume(cur, t, N, threshold, max_o, max_e, hit, unknown);
      cur = nx;
      hit = (hit || lost || (unknown_hits && unknown)) && active;
      unknown = unknown && active;
      hit_any = hit_any || hit;
      unknown_any = unknown_any || unknown;
      const unsigned long long hitting = __ballot(hit), unknowing = __ballot(unknown);
      if (lane == 0 && (hitting | unknowing)) atomicAdd(&cnt[t], __popcll(hitting) | (__popcll(unknowing) << 16));
    }
  }

  // ---- reduction: butterflies inside the wavefronts, then the wavefronts in order by one lane
  const Place z = place_of(threads);
  const Lds e = lds_layout(lds, z.N);
  int max_r = active && max_e != NO_INDEX ? z.s0 + tid : NO_INDEX;
  if (max_r == NO_INDEX) { max_o = -__builtin_huge_val(); max_e = NO_INDEX; }
  wave_row_merge(max_o, max_r, max_e);
  const int wave_hits = __popcll(__ballot(hit_any)), wave_unknown = __popcll(__ballot(unknown_any));
  if (lane == 0) { e.red_o[wave] = max_o; e.red_r[wave] = max_r; e.red_e[wave] = max_e; e.red_h[wave] = wave_hits; e.red_u[wave] = wave_unknown; }
  __syncthreads();  // (every counter is final)
  if (tid == 0) {
    int hit_rows = wave_hits, unknown_rows = wave_unknown;
    const int waves = threads / WAVE;
    for (int v = 1; v < waves; ++v) {
      row_merge(max_o, max_r, max_e, e.red_o[v], e.red_r[v], e.red_e[v]);
      hit_rows += e.red_h[v];
      unknown_rows += e.red_u[v];
    }
    e.rec[0] = (double)hit_rows; e.rec[1] = max_o; e.rec[2] = (double)max_r; e.rec[3] = (double)max_e; e.rec[4] = (double)unknown_rows;
  }
  __syncthreads();
  const MapRiskArgs& q = risk_args();
  if (z.G == 1) {  // one record per solve: the first wavefront writes the outputs itself, from LDS, by the finish kernel's statements
    if (wave == 0) map_risk_finish(q, z.b, 1, lane, e.rec, e.cnt, 0);
    return;
  }
  double* part = q.r.partials + (long long)blockIdx.x * q.r.part_stride;
  int32_t* pc = reinterpret_cast<int32_t*>(part + RISK_PART_DOUBLES);
  for (int t = tid; t < z.N; t += threads) pc[t] = e.cnt[t];
  if (tid < 5) part[tid] = e.rec[tid];
}

// G > 1: one wavefront per solve joins its G partial records in ascending order.
__global__ __launch_bounds__(WAVE) void cilqr_rollout_risk_map_finish_kernel(MapRiskArgs a) {
  const MapRiskArgs& q = risk_args();
  const int b = blockIdx.x, G = q.r.G;
  const double* part = q.r.partials + (long long)b * G * q.r.part_stride;
  map_risk_finish(q, b, G, threadIdx.x, part, reinterpret_cast<const int32_t*>(part + RISK_PART_DOUBLES), q.r.part_stride);
}

}  // namespace

size_t rollout_risk_map_lds_bytes(int N) {
  return ((size_t)N * NOM_W + 4 + RISK_WAVES + RISK_PART_DOUBLES) * sizeof(double) + ((size_t)N + 4 * RISK_WAVES) * sizeof(int32_t);
}

hipError_t launch_rollout_risk_map(const MapRiskArgs& a, hipStream_t stream) {
  return launch_risk_pair(cilqr_rollout_risk_map_kernel, cilqr_rollout_risk_map_finish_kernel, a, a.r.s.B, a.r.S, a.r.G,
                          rollout_risk_map_lds_bytes(a.r.s.N), stream);
}

}  // namespace cilqr
