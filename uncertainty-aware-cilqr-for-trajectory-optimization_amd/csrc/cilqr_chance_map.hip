// cilqr_chance_map.hip — analytic map risk (cilqr_chance_risk_map*, include/cilqr.h): per step the pose marginal (x, y, theta) of
// Sigma_t is factored, Q weighted standard-normal nodes are placed through the factor around the plan's pose, and the footprint is
// looked up under every node pose with the probes and the bilinear lookup of the map cost (cilqr_map_probes.hpp).  Per step: the
// weighted mass of nodes that hit, of nodes that are unknown, and the weighted mean of the nodes' largest occupancy.
//
// Why the mapping differs from cilqr_risk_map.hip.  There a row is a closed-loop rollout: a serial chain over the horizon, so the
// step is the inner loop and a solve has ceil(S/256) workgroups.  Here Sigma_t is an input: the N·Q node poses of a solve depend
// on nothing but X_t, six entries of Sigma_t and the node, so the steps go to different wavefronts.  lane = node in chunks of 64,
// wavefront = step, a workgroup of CHANCE_MAP_WAVES wavefronts takes as many consecutive steps of ONE solve, solve b has
// G = ceil(N / CHANCE_MAP_WAVES) workgroups, the grid is B·G.  The nodes and weights (32 bytes per node) are staged once per
// workgroup in LDS; the step's pose and factor are wavefront-uniform values every lane forms from the same nine loads and moves to
// scalar registers (uniform_double).
//
// Sums.  A lane adds its chunks' terms in ascending q; the 64 lane sums then go through a fixed xor butterfly (every lane ends with
// the same bits: the additions of a level are commutative pairs).  The tree is fixed by Q alone.  The step's largest occupancy is
// a maximum.  Lane 0 writes r_t, u_t, e_t to the caller's per-step arrays, or to the handle's where the caller passed none; the
// workgroup's largest occupancy goes to its slot of the handle's partial records.  The reduction over t — fields 0..7 and `total`
// — is the finish kernel's: one wavefront per solve, lane sums over t ascending and the same butterfly (a tree fixed by N),
// lexicographic maxima.  No atomics anywhere.
//
// Load scheduling is the one of cilqr_risk_map.hip: the probes are taken in groups of PROBE_GROUP, a group's loads are issued
// together and unconditionally, and a group is consumed only after the next group's loads are in flight; the first group of the
// NEXT chunk's node leaves (after that node's sincos) before the last group of this chunk's node is used.
// No scratch memory, no spilled register, 128 vector registers at most (make check).
#include "cilqr_map_probes.hpp"

namespace cilqr {

using namespace dev;

namespace {

__device__ __forceinline__ const ChanceMapArgs& map_args() { return const_kernel_args<ChanceMapArgs>(); }

// The step's factor: the lower Cholesky factor of the (x, y, theta) marginal, zero where a pivot vanishes (include/cilqr.h).
struct Factor {
  double l00, l10, l11, l20, l21, l22;
};
__device__ __forceinline__ Factor pose_factor(double c00, double c10, double c11, double c20, double c21, double c22) {
#pragma clang fp contract(off)
  Factor f;
  f.l00 = sqrt(fmax(c00, 0.0));
  f.l10 = f.l00 > 0.0 ? c10 / f.l00 : 0.0;
  f.l20 = f.l00 > 0.0 ? c20 / f.l00 : 0.0;
  f.l11 = sqrt(fmax(c11 - f.l10 * f.l10, 0.0));
  f.l21 = f.l11 > 0.0 ? (c21 - f.l20 * f.l10) / f.l11 : 0.0;
  f.l22 = sqrt(fmax(c22 - f.l20 * f.l20 - f.l21 * f.l21, 0.0));
  return f;
}

struct NodePose {
  double x, y, c, s, w;  // position, cos and sin of the heading, the node's weight (0 for a lane beyond Q)
};
// Node q of the chunk: the step's pose displaced through the factor.  A lane beyond Q sits on the mean with weight 0.
__device__ __forceinline__ NodePose node_pose(const double* nodes, const double* weights, int q, int Q, double mx, double my, double mth,
                                              const Factor& f) {
#pragma clang fp contract(off)
  double zx = 0.0, zy = 0.0, zt = 0.0;
  NodePose p;
  p.w = 0.0;
  if (q < Q) { zx = nodes[3 * q]; zy = nodes[3 * q + 1]; zt = nodes[3 * q + 2]; p.w = weights[q]; }
  p.x = mx + f.l00 * zx;
  p.y = my + (f.l10 * zx + f.l11 * zy);
  const double th = mth + (f.l20 * zx + f.l21 * zy + f.l22 * zt);
  sincos_fast(th, &p.s, &p.c);
  return p;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {  // (a NaN never enters: occupancies that reach here are finite or -inf)
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
  return v;
}

// LDS (dynamic): [nodes: 3·Q][weights: Q][largest occupancy per wavefront: CHANCE_MAP_WAVES]
__global__ __launch_bounds__(CHANCE_MAP_THREADS) void cilqr_chance_risk_map_kernel(ChanceMapArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int N = a.s.N, Q = a.Q, G = a.G;
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int t = g * CHANCE_MAP_WAVES + wave;  // (wavefront-uniform)
  double* nodes = lds;
  double* weights = lds + 3 * (size_t)Q;
  double* red = weights + Q;
  for (int i = tid; i < 3 * Q; i += CHANCE_MAP_THREADS) nodes[i] = a.nodes[i];
  for (int i = tid; i < Q; i += CHANCE_MAP_THREADS) weights[i] = a.weights[i];
  __syncthreads();

  double worst = -__builtin_huge_val();
  if (t < N) {  // (a workgroup's last wavefronts idle where N is no multiple of CHANCE_MAP_WAVES)
    const double* X = a.X + ((size_t)b * (N + 1) + t) * 4;
    const double* S = a.sigma + ((size_t)b * (N + 1) + t) * 16;
    const double mx = X[0], my = X[1], mth = X[3];
    const double c00 = S[0], c10 = S[4], c11 = S[5], c20 = S[12], c21 = S[13], c22 = S[15];  // (r, c) at [r + 4c], row <= column
    const bool lost = !(is_finite(mx) && is_finite(my) && is_finite(mth) && is_finite(c00) && is_finite(c10) && is_finite(c11) &&
                        is_finite(c20) && is_finite(c21) && is_finite(c22));
    double r = 1.0, un = 1.0, e = 0.0;
    if (!lost) {
      Factor f = pose_factor(c00, c10, c11, c20, c21, c22);
      f.l00 = uniform_double(f.l00); f.l10 = uniform_double(f.l10); f.l11 = uniform_double(f.l11);
      f.l20 = uniform_double(f.l20); f.l21 = uniform_double(f.l21); f.l22 = uniform_double(f.l22);
      UncPose po = unc_pose(map_args().s.unc, b);
      po.px = uniform_double(po.px); po.py = uniform_double(po.py); po.cp = uniform_double(po.cp); po.sp = uniform_double(po.sp);
      const LayerPtr layer = (LayerPtr)(map_args().s.unc.layer + (size_t)b * (size_t)map_args().s.unc.stride);
      const int P = map_args().s.unc.nl * map_args().s.unc.nw;
      const bool unknown_hits = (map_args().flags & CILQR_CHANCE_MAP_UNKNOWN_HITS) != 0;
      const int chunks = (Q + WAVE - 1) / WAVE;
      double acc_r = 0.0, acc_u = 0.0, acc_e = 0.0;
      // the first group of the first chunk leaves; from here on `cur` is a group whose loads are in flight
      NodePose np = node_pose(nodes, weights, lane, Q, mx, my, mth, f);
      int k = 0, l = 0;
      ProbeGroup cur;
      probes_issue(map_args().s.unc, po, layer, np.x, np.y, np.c, np.s, true, 0, k, l, cur);
      for (int c = 0; c < chunks; ++c) {
        bool hit = false, unknown = false;
        double max_o = -__builtin_huge_val();
        int max_e = NO_INDEX;
        for (int q0 = PROBE_GROUP; q0 < P; q0 += PROBE_GROUP) {  // the next group's loads leave before this group's are used
          ProbeGroup nx;
          probes_issue(map_args().s.unc, po, layer, np.x, np.y, np.c, np.s, true, q0, k, l, nx);
          probes_consume(cur, 0, 1, map_args().occ_threshold, max_o, max_e, hit, unknown);
          cur = nx;
        }
        // the next chunk's node and its first group leave before the last group of this one is used
        const double w = np.w;
        ProbeGroup nx = {};
        k = 0; l = 0;
        if (c + 1 < chunks) {
          np = node_pose(nodes, weights, (c + 1) * WAVE + lane, Q, mx, my, mth, f);
          probes_issue(map_args().s.unc, po, layer, np.x, np.y, np.c, np.s, true, 0, k, l, nx);
        }
        probes_consume(cur, 0, 1, map_args().occ_threshold, max_o, max_e, hit, unknown);
        cur = nx;
        hit = hit || (unknown_hits && unknown);
        // (a lane beyond Q has weight 0 and adds +0; its occupancy is the mean pose's and must not enter the maximum)
        const bool counts = c * WAVE + lane < Q;
        const bool any = max_e != NO_INDEX;
        acc_r += hit && counts ? w : 0.0;
        acc_u += unknown && counts ? w : 0.0;
        acc_e += any && counts ? w * max_o : 0.0;
        if (any && counts) worst = fmax(worst, max_o);
      }
      acc_r = wave_sum(acc_r); acc_u = wave_sum(acc_u); e = wave_sum(acc_e);
      r = !(acc_r <= 1.0) ? 1.0 : acc_r;  // (a sum that is NaN gives 1: weights the device form cannot check)
      un = !(acc_u <= 1.0) ? 1.0 : acc_u;
      worst = wave_max(worst);
    }
    if (lane == 0) {
      const size_t at = (size_t)b * N + t;
      const ChanceMapArgs& z = map_args();  // (read anew: carried across the node loop these pointers would be spilled)
      z.step_risk[at] = r; z.step_unknown[at] = un; z.step_occ[at] = e;
    }
  }
  if (lane == 0) red[wave] = worst;
  __syncthreads();
  if (tid == 0) {
    double m = red[0];
#pragma unroll
    for (int v = 1; v < CHANCE_MAP_WAVES; ++v) m = fmax(m, red[v]);
    map_args().partials[(size_t)b * map_args().part_stride + g] = m;
  }
}

// (max value, lowest step); a NaN never wins
__device__ __forceinline__ void step_merge(double& c0, int& t0, double c1, int t1) {
  if (c1 > c0 || (c1 == c0 && t1 < t0)) { c0 = c1; t0 = t1; }
}

// One wavefront per solve: the per-step values and the G workgroup maxima → risk [CILQR_CHANCE_MAP_FIELDS] and total.
__global__ __launch_bounds__(WAVE) void cilqr_chance_risk_map_finish_kernel(ChanceMapArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, N = a.s.N, G = a.G;
  const double* sr = a.step_risk + (size_t)b * N;
  const double* su = a.step_unknown + (size_t)b * N;
  const double* se = a.step_occ + (size_t)b * N;
  const double* part = a.partials + (size_t)b * a.part_stride;
  double max_r = -__builtin_huge_val(), max_e = -__builtin_huge_val(), max_u = -__builtin_huge_val(), sum = 0.0;
  double worst = -__builtin_huge_val();
  int at_r = NO_INDEX, at_e = NO_INDEX, first = NO_INDEX;
  for (int t = lane; t < N; t += WAVE) {  // ascending t within the lane
    const double r = sr[t];
    step_merge(max_r, at_r, r, t);
    step_merge(max_e, at_e, se[t], t);
    max_u = fmax(max_u, su[t]);
    sum += r;
    if (r > 0.0) first = min(first, t);
  }
  for (int g = lane; g < G; g += WAVE) worst = fmax(worst, part[g]);
  for (int o = 32; o > 0; o >>= 1) {
    step_merge(max_r, at_r, __shfl_xor(max_r, o, WAVE), __shfl_xor(at_r, o, WAVE));
    step_merge(max_e, at_e, __shfl_xor(max_e, o, WAVE), __shfl_xor(at_e, o, WAVE));
    max_u = fmax(max_u, __shfl_xor(max_u, o, WAVE));
    worst = fmax(worst, __shfl_xor(worst, o, WAVE));
    first = min(first, __shfl_xor(first, o, WAVE));
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    const double sum_risk = sum > 1.0 ? 1.0 : sum;
    double* out = a.risk + (size_t)b * CILQR_CHANCE_MAP_FIELDS;
    out[CILQR_CM_STEP_RISK] = max_r;
    out[CILQR_CM_WORST_STEP] = at_r == NO_INDEX ? -1.0 : (double)at_r;
    out[CILQR_CM_SUM_RISK] = sum_risk;
    out[CILQR_CM_FIRST_STEP] = first == NO_INDEX ? -1.0 : (double)first;
    out[CILQR_CM_MEAN_OCC] = max_e;
    out[CILQR_CM_MEAN_OCC_STEP] = at_e == NO_INDEX ? -1.0 : (double)at_e;
    out[CILQR_CM_WORST_OCC] = worst;
    out[CILQR_CM_UNKNOWN] = max_u;
    if (a.total) {
      const double base = a.base[b];
      const double bounded = (a.flags & CILQR_CHANCE_MAP_BOUND_SUM) ? sum_risk : max_r;
      a.total[b] = is_finite(base) && !(bounded > a.max_risk) ? base : __builtin_nan("");
    }
  }
}

}  // namespace

size_t chance_risk_map_lds_bytes(int Q) { return ((size_t)4 * Q + CHANCE_MAP_WAVES) * sizeof(double); }

hipError_t launch_chance_risk_map(const ChanceMapArgs& a, hipStream_t stream) {
  if (a.s.B <= 0 || a.s.N <= 0) return hipSuccess;
  const long long blocks = (long long)a.s.B * a.G;
  hipLaunchKernelGGL(cilqr_chance_risk_map_kernel, dim3((unsigned)blocks), dim3(CHANCE_MAP_THREADS), chance_risk_map_lds_bytes(a.Q), stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_chance_risk_map_finish_kernel, dim3(a.s.B), dim3(WAVE), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
