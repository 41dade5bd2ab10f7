/* device_math_model.c — TEST INFRASTRUCTURE ONLY.
 *
 * Operation-for-operation restatements of two device routines of the product's csrc/cilqr_device.hpp, exp_full (exp_fast and the select of its low end) and rotate_heading,
 * in IEEE arithmetic on the host: every fused multiply-add is libm's fma (exact, one rounding), every other operation a single
 * multiplication, rint or ldexp, and the file is compiled with -ffp-contract=off, so nothing is fused that is not written fused and
 * nothing written fused is split.  Both routines are written that way on the device too, so the device is expected to return these
 * bits (tests/test_device_math.py asserts it); against mpmath the model is checked on the CPU.
 *
 * Nothing here is shared with the product: the constants are typed again from the same decimal literals and quotients.
 */
#include <limits.h>
#include <math.h>

/* double -> int32 as the device converts: saturating, NaN -> 0 (a plain C cast is undefined there) */
static int cvt_i32(double n) {
  if (n != n) return 0;
  if (n >= 2147483647.0) return INT_MAX;
  if (n <= -2147483648.0) return INT_MIN;
  return (int)n;
}

static double model_exp_one(double x) {
  const double n = rint(x * 1.44269504088896338700e+00);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const double e = ldexp(p, cvt_i32(n));
  const double lo = x < -746.0 ? 0.0 : e;
  return x > 710.0 ? HUGE_VAL : lo;
}

void model_exp_full(int n, const double* x, double* out) {
  for (int i = 0; i < n; ++i) out[i] = model_exp_one(x[i]);
}

/* n chains of T steps: sc0 = n x (sin, cos) of the first heading, delta = n x T turns, out = n x T x (sin, cos) */
void model_rotate_heading(int n, int T, const double* sc0, const double* delta, double* out) {
  const double sn1 = -1.0 / 6.0, sn2 = 1.0 / 120.0, sn3 = -1.0 / 5040.0, sn4 = 1.0 / 362880.0, sn5 = -1.0 / 39916800.0;
  const double cs1 = -0.5, cs2 = 1.0 / 24.0, cs3 = -1.0 / 720.0, cs4 = 1.0 / 40320.0, cs5 = -1.0 / 3628800.0, cs6 = 1.0 / 479001600.0;
  for (int i = 0; i < n; ++i) {
    double sn = sc0[2 * i], cs = sc0[2 * i + 1];
    for (int t = 0; t < T; ++t) {
      const double d = delta[(long)i * T + t];
      const double z = d * d;
      double ps = fma(z, sn5, sn4);
      double pc = fma(z, cs6, cs5);
      pc = fma(pc, z, cs4);
      ps = fma(ps, z, sn3);
      pc = fma(pc, z, cs3);
      ps = fma(ps, z, sn2);
      pc = fma(pc, z, cs2);
      ps = fma(ps, z, sn1);
      pc = fma(pc, z, cs1);
      const double sd = fma(d * z, ps, d);
      const double cdm1 = pc * z;
      const double c0 = cs, s0 = sn;
      cs = fma(c0, cdm1, fma(-s0, sd, c0));
      sn = fma(s0, cdm1, fma(c0, sd, s0));
      out[((long)i * T + t) * 2] = sn;
      out[((long)i * T + t) * 2 + 1] = cs;
    }
  }
}
