// cilqr_chance_entry.hpp — the chance value of one obstacle entry under Σ_t, ONE definition for the kernels that form it
// (cilqr_chance.hip: ordinary obstacles, one workgroup per solve; cilqr_chance_sampled.hip: sampled obstacles in compact form,
// wavefront = step).  The bit-equality the tests assert — the sampled call's entry_p == cilqr_chance_risk's on the materialised
// table — holds because both kernels form the entry by make_obs_entry and the argument by the statements below.
#pragma once

#include "cilqr_rollout_core.hpp"

namespace cilqr {
namespace dev {

// One ego circle against one entry: c = 1 - d'Pd by the statements of circle_constraints (cilqr_score.hip), its gradient over the
// circle centre g_xy = -2 R(θ_o)' P d (I/Obstacle.cpp:82, 101), and under Σ = {xx, xy, xθ, yy, yθ, θθ} the argument z of the chance
// value p = erfc(z)/2: z = -c̄/(s√2), or with s = 0 the infinity that gives p = 1 (c̄ > 0) or 0.  (lx, ly) = d(centre)/dθ =
// (-ℓ sin θ, ℓ cos θ).
// FRONT: the front circle (lever +ℓ: lx is the negated product), else the rear one (lever -ℓ: ly is).
struct ChanceForm {  // c̄, the form g'Σg, and g's position components
  double c, q, gx, gy;
};
template <bool FRONT>
__device__ __forceinline__ ChanceForm circle_chance_form(const ObsEntry& e, double cx, double cy, double lx, double ly, const double* S) {
  ChanceForm f;
  {
#pragma clang fp contract(off)
    const double ex = cx - e.ox, ey = cy - e.oy;
    const double d0 = __builtin_fma(e.co, ex, e.so * ey);
    const double d1 = __builtin_fma(e.co, ey, -(e.so * ex));
    f.c = 1 - __builtin_fma(d0 * e.ia2, d0, (d1 * e.ib2) * d1);
    const double p0 = d0 * e.ia2, p1 = d1 * e.ib2;
    const double gx = -2 * (e.co * p0 - e.so * p1);
    const double gy = -2 * (e.so * p0 + e.co * p1);
    // g'Σg with every fused multiply-add written out — the ones the compiler chose for cilqr_chance.hip while contraction was left
    // to it: of gt's two products it rounded the one whose lever component is the negated product and fused the other, so the
    // circles differ.  (Left to it again, it chose otherwise in cilqr_chance_sampled.hip: the bits must not depend on that.)
    const double gt = FRONT ? __builtin_fma(gy, ly, gx * lx) : __builtin_fma(gx, lx, gy * ly);
    const double sq = __builtin_fma(gt * gt, S[5], __builtin_fma(gx * gx, S[0], (gy * gy) * S[3]));
    const double cr = __builtin_fma(gy * gt, S[4], __builtin_fma(gx * gy, S[1], (gx * gt) * S[2]));
    f.q = __builtin_fma(2.0, cr, sq);
    f.gx = gx; f.gy = gy;
  }
  return f;
}
// The form with the obstacle's own position covariance C = {xx, xy, yy} (world frame, independent of the ego's error) added:
// g_xy' C g_xy, its fused multiply-adds written out like the ones above (cilqr_chance_risk_cov).
__device__ __forceinline__ double chance_form_with_cov(const ChanceForm& f, double cxx, double cxy, double cyy) {
#pragma clang fp contract(off)
  return f.q + __builtin_fma(2.0 * (f.gx * f.gy), cxy, __builtin_fma(f.gx * f.gx, cxx, (f.gy * f.gy) * cyy));
}
__device__ __forceinline__ double chance_arg(double c, double q) {
  const double s = sqrt(fmax(q, 0.0));  // (fmax: a NaN form counts as 0)
  if (!(s > 0.0)) return c > 0.0 ? -__builtin_huge_val() : __builtin_huge_val();
  return -c / (s * 1.41421356237309514547e+00);
}
template <bool FRONT>
__device__ __forceinline__ double circle_chance_arg(const ObsEntry& e, double cx, double cy, double lx, double ly, const double* S) {
  const ChanceForm f = circle_chance_form<FRONT>(e, cx, cy, lx, ly, S);
  return chance_arg(f.c, f.q);
}

}  // namespace dev
}  // namespace cilqr
