// host_plan_predict.cpp — do the host forms of cilqr_predict_obstacles and cilqr_chance_risk_cov fit the arena cilqr_create reserves,
// at the shapes include/cilqr.h says always fit, and is that arena still the one the earlier calls sized?  Plain C++ over
// csrc/cilqr_host_plan.h, no HIP.  Laid out without an arena (sizes and offsets only):
//   plan_predict_obstacles  - with every output at T = max_batch / 8, N = max_horizon, M = max_obstacles (M >= 1),
//                           - without sigma_out at T = max_batch / 5,
//   plan_chance_risk_cov    - dense obstacles with obs_cov, a shared or a per-solve sigma0 and process noise, at B = max_batch / 2 with
//                             and without sigma_out and entry_p,
// each end compared with host_arena_bytes(max_batch, max_horizon, max_obstacles); the prediction with every output at T = max_batch
// is reported (it need not fit: the call then returns CILQR_ERR_ARG).  For every (B, N, M) triple on the command line it prints
// host_arena_bytes, which the test compares with tests/golden/host_arena_cap.json.
// Prints one line per reported shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static size_t predict_end(size_t T, size_t N, size_t M, bool with_sigma, int* n_arrays, bool* ok) {
  static double host;
  const double *track = &host, *dim = &host, *cov = &host, *noise = &host;
  double *pose = &host, *dim_out = &host, *cov_out = &host, *sigma = with_sigma ? &host : nullptr;
  cilqr::HostPlan p(nullptr);
  cilqr::plan_predict_obstacles(p, T, N, M, track, dim, cov, noise, pose, dim_out, cov_out, sigma);
  *n_arrays = p.n;
  *ok = p.ok;
  return p.end;
}

static size_t chance_cov_end(size_t B, size_t N, size_t M, bool per_solve, bool all, int* n_arrays, bool* ok) {
  static double host;
  const double *X = &host, *U = &host, *K = &host, *s0 = &host, *W = &host, *base = &host, *oc = M ? &host : nullptr;
  double *risk = &host, *step = &host, *ep = all ? &host : nullptr, *so = all ? &host : nullptr, *total = &host;
  cilqr_obstacles o = {&host, &host, &host, 0, 0, 0, 0};
  cilqr::HostPlan p(nullptr);
  cilqr::plan_chance_risk_cov(p, B, N, M, per_solve ? B : 1, X, U, K, s0, W, o, B * M * N, oc, base, risk, step, ep, so, total);
  *n_arrays = p.n;
  *ok = p.ok;
  return p.end;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 5, 8, 15, 16, 64, 1024, 4096}, horizons[] = {1, 2, 12, 50, 383, CILQR_MAX_HORIZON}, obstacles[] = {0, 1, 4, 64, 1024};
  int bad = 0, n = 0, most = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles) {
        const size_t cap = cilqr::host_arena_bytes(B, N, M);
        const bool show = B == 1024 && N == 50 && M == 4;
        int arrays = 0;
        bool ok = false;
        if (M >= 1) {
          if (B / 8 >= 1) {
            const size_t full = predict_end(B / 8, N, M, true, &arrays, &ok);
            const bool fits = ok && arrays == 8 && full <= cap;
            ++n;
            if (!fits || show) printf("predict T %zu of max_batch %zu, N %zu M %zu, every output: plan %zu of %zu bytes, %d arrays%s\n", B / 8, B, N, M, full, cap, arrays, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          }
          if (B / 5 >= 1) {
            const size_t lean = predict_end(B / 5, N, M, false, &arrays, &ok);
            const bool fits = ok && arrays == 7 && lean <= cap;
            ++n;
            if (!fits || show) printf("predict T %zu of max_batch %zu, N %zu M %zu, no sigma_out: plan %zu of %zu bytes, %d arrays%s\n", B / 5, B, N, M, lean, cap, arrays, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          }
          const size_t whole = predict_end(B, N, M, true, &arrays, &ok);
          if (show) printf("predict T %zu N %zu M %zu, every output: plan %zu of %zu bytes (%s)\n", B, N, M, whole, cap, whole <= cap ? "fits" : "CILQR_ERR_ARG");
        }
        if (B / 2 >= 1)
          for (int per_solve = 0; per_solve < 2; ++per_solve)
            for (int all = 0; all < 2; ++all) {
              const size_t end = chance_cov_end(B / 2, N, M, per_solve, all, &arrays, &ok);
              const int expect = (all ? (M ? 13 : 10) : (M ? 11 : 9)) + (M ? 1 : 0);
              const bool fits = ok && arrays == expect && end <= cap;
              if (arrays > most) most = arrays;
              ++n;
              if (!fits || show) printf("chance_risk_cov B %zu of max_batch %zu, N %zu M %zu, %s sigma0, %s: plan %zu of %zu bytes, %d arrays%s\n", B / 2, B, N, M, per_solve ? "per-solve" : "shared", all ? "every output" : "no sigma_out / entry_p", end, cap, arrays, fits ? "" : "  DOES NOT FIT");
              bad += !fits;
            }
      }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), %d arrays at most of %d\n", n, most, (int)cilqr::HostPlan::CAP);
  return 0;
}
