// cilqr_map_probes.hpp — the footprint probes and the bilinear lookup of the uncertainty map as the risk kernels take them
// (cilqr_risk_map.hip: under rollout states; cilqr_chance_map.hip: under quadrature nodes): the statements of unc_cost_add
// (cilqr_device.hpp) split into the half before a probe's four loads and the half after them, so that a group's loads are in flight
// while something else is computed.  Probe positions, cell indices, the validity test and the interpolant are restated with
// contraction off: the occupancy is bit-equal to the one the map cost interpolates at that probe.
#pragma once

#include "cilqr_rollout_core.hpp"

namespace cilqr {
namespace dev {

constexpr int PROBE_GROUP = 3;  // probes whose 4·PROBE_GROUP loads are issued together: what 128 vector registers hold twice

typedef const __attribute__((address_space(1))) float* LayerPtr;  // the layer lies in global memory: global loads, not flat ones

// kernel_args (cilqr_rollout_core.hpp) with the pointer kept in the CONSTANT address space: what is read through it — the map's
// constants, the dynamics' parameters — comes by scalar loads, which no store of the kernel can be thought to clobber and whose waits
// (lgkmcnt) do not wait for the layer's vector loads (vmcnt).  Read where a probe group uses them, the constants are not carried
// across the step or node loop, where they would not fit the scalar registers.
template <class A>
__device__ __forceinline__ const A& const_kernel_args() {
  const __attribute__((address_space(4))) A* q = (const __attribute__((address_space(4))) A*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(q));
  return *(const A*)q;
}

// A wavefront-uniform double moved to scalar registers (the map pose: a per-solve pose is formed by vector instructions).
__device__ __forceinline__ double uniform_double(double v) {
  const unsigned long long w = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)w), hi = __builtin_amdgcn_readfirstlane((unsigned)(w >> 32));
  return __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

// PROBE_GROUP probes between their loads and their use.  `exists`: bit i set when probe q0 + i is one of the footprint's;
// `inside`: its four cells lie inside the map (the loads of a probe that is not inside read cells (0,0)..(1,1)).
struct ProbeGroup {
  float f00[PROBE_GROUP], f10[PROBE_GROUP], f01[PROBE_GROUP], f11[PROBE_GROUP];
  double ti[PROBE_GROUP], tj[PROBE_GROUP];
  int q0;
  unsigned exists, inside;
};

// Probes q0 .. q0 + PROBE_GROUP - 1 of the state (x, y, cos ct, sin st), q = k·probes_w + l; (k, l) is probe q0's on entry and
// probe (q0 + PROBE_GROUP)'s on return; state_finite: the state's speed is finite.  The statements of unc_cost_add up to its loads.
__device__ __forceinline__ void probes_issue(const UncArgs& u, const UncPose& po, LayerPtr layer, double x, double y, double ct, double st,
                                             bool state_finite, int q0, int& k, int& l, ProbeGroup& g) {
#pragma clang fp contract(off)  // probe positions and cell indices as the plain-C statement forms them
  const int rows = u.rows, cols = u.cols, nw = u.nw, P = u.nl * nw;
  g.q0 = q0; g.exists = 0; g.inside = 0;
#pragma unroll
  for (int i = 0; i < PROBE_GROUP; ++i) {
    g.f00[i] = g.f10[i] = g.f01[i] = g.f11[i] = 0.0f;
    g.ti[i] = g.tj[i] = 0.0;
    if (q0 + i < P) {  // (uniform)
      const double a = u.la0 + (double)k * u.la_step;
      const double bb = u.wb0 + (double)l * u.wb_step;
      const double Px = x + (a * ct - bb * st), Py = y + (a * st + bb * ct);
      const double dx = Px - po.px, dy = Py - po.py;
      const double qx = po.cp * dx + po.sp * dy, qy = po.cp * dy - po.sp * dx;
      const double fi = (u.x_first - qx) * u.inv_res, fj = (u.y_first - qy) * u.inv_res;
      // (a state that is not finite has no valid probe: x, y and the heading fail the comparisons by themselves, the speed is asked)
      const bool in = state_finite && !(!(fi >= 0.0) || !(fj >= 0.0) || !(fi < (double)(rows - 1)) || !(fj < (double)(cols - 1)));
      const int i0 = in ? (int)fi : 0, j0 = in ? (int)fj : 0;
      g.ti[i] = fi - (double)i0; g.tj[i] = fj - (double)j0;
      const LayerPtr c0 = layer + (size_t)j0 * rows + i0;
      g.f00[i] = c0[0]; g.f10[i] = c0[1]; g.f01[i] = c0[rows]; g.f11[i] = c0[rows + 1];
      g.exists |= 1u << i;
      g.inside |= in ? 1u << i : 0u;
      if (++l == nw) { l = 0; ++k; }
    }
  }
}

// The group's occupancies at step t of N: the validity test and the interpolant of unc_cost_add.  A valid probe enters the row's
// (max, lowest entry) and hits above the threshold; an invalid one makes the row unknown at this step.
__device__ __forceinline__ void probes_consume(const ProbeGroup& g, int t, int N, double threshold, double& max_o, int& max_e, bool& hit,
                                               bool& unknown) {
#pragma clang fp contract(off)  // the interpolant decides a hit
#pragma unroll
  for (int i = 0; i < PROBE_GROUP; ++i) {
    if (g.exists >> i & 1u) {  // (uniform)
      const double f00 = g.f00[i], f10 = g.f10[i], f01 = g.f01[i], f11 = g.f11[i];
      const double ti = g.ti[i], tj = g.tj[i];
      const double big = 1.0e300;  // finite test without library calls (NaN fails every comparison)
      const bool valid = (g.inside >> i & 1u) && fabs(f00) < big && fabs(f10) < big && fabs(f01) < big && fabs(f11) < big;
      const double a0 = f00 + ti * (f10 - f00), a1 = f01 + ti * (f11 - f01);
      const double o = a0 + tj * (a1 - a0);
      if (valid) {
        cmax_merge(max_o, max_e, o, (g.q0 + i) * N + t);
        hit = hit || o > threshold;
      } else {
        unknown = true;
      }
    }
  }
}

}  // namespace dev
}  // namespace cilqr
