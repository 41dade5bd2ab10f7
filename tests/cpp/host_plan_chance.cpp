// host_plan_chance.cpp — does the host form of cilqr_chance_risk fit the arena cilqr_create reserves, at the shapes include/cilqr.h
// says always fit, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h, no HIP:
// plan_chance_risk is laid out without an arena (sizes and offsets only) with dense obstacles, a shared or a per-solve sigma0 and
// process noise,
//   - without sigma_out and entry_p at B = max_batch, N = max_horizon, M = max_obstacles,
//   - with every output asked for at B = max_batch / 2,
// and its end is compared with host_arena_bytes(max_batch, max_horizon, max_obstacles); the plan with every output at B = max_batch
// is reported (it need not fit: the call then returns CILQR_ERR_ARG).  For every (B, N, M) triple on the command line it prints
// host_arena_bytes, which the test compares with tests/golden/host_arena_cap.json: the arena is the one the earlier calls sized.
// Prints one line per reported shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static size_t plan_end(size_t B, size_t N, size_t M, bool per_solve, bool all, int* n_arrays, bool* ok) {
  static double host;
  const double *X = &host, *U = &host, *K = &host, *s0 = &host, *W = &host, *base = &host;
  double *risk = &host, *step = &host, *ep = all ? &host : nullptr, *so = all ? &host : nullptr, *total = &host;
  cilqr_obstacles o = {&host, &host, &host, 0, 0, 0, 0};
  cilqr::HostPlan p(nullptr);
  cilqr::plan_chance_risk(p, B, N, M, per_solve ? B : 1, X, U, K, s0, W, o, B * M * N, base, risk, step, ep, so, total);
  *n_arrays = p.n;
  *ok = p.ok;
  return p.end;
}

int main(int argc, char** argv) {
  // "arena B N M = bytes" for every (B, N, M) given on the command line: the caller compares them with recorded values
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 15, 16, 64, 1024, 4096}, horizons[] = {1, 2, 12, 50, 383, CILQR_MAX_HORIZON}, obstacles[] = {0, 1, 4, 64};
  int bad = 0, n = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles) {
        const size_t cap = cilqr::host_arena_bytes(B, N, M);
        for (int per_solve = 0; per_solve < 2; ++per_solve) {
          int arrays = 0;
          bool ok = false;
          const size_t lean = plan_end(B, N, M, per_solve, false, &arrays, &ok);
          const int lean_arrays = M ? 11 : 9;
          bool fits = ok && arrays == lean_arrays && lean <= cap;
          ++n;
          if (!fits || (B == 1024 && N == 50 && M == 4)) printf("B %zu N %zu M %zu, %s sigma0, no sigma_out / entry_p: plan %zu of %zu bytes, %d arrays%s\n", B, N, M, per_solve ? "per-solve" : "shared", lean, cap, arrays, fits ? "" : "  DOES NOT FIT");
          bad += !fits;
          if (B / 2 >= 1) {
            const size_t half = plan_end(B / 2, N, M, per_solve, true, &arrays, &ok);
            fits = ok && arrays == (M ? 13 : 10) && half <= cap;
            ++n;
            if (!fits || (B == 1024 && N == 50 && M == 4)) printf("B %zu of max_batch %zu, N %zu M %zu, %s sigma0, every output: plan %zu of %zu bytes, %d arrays%s\n", B / 2, B, N, M, per_solve ? "per-solve" : "shared", half, cap, arrays, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          }
          const size_t full = plan_end(B, N, M, per_solve, true, &arrays, &ok);
          if (B == 1024 && N == 50 && M == 4) printf("B %zu N %zu M %zu, %s sigma0, every output: plan %zu of %zu bytes (%s)\n", B, N, M, per_solve ? "per-solve" : "shared", full, cap, full <= cap ? "fits" : "CILQR_ERR_ARG");
        }
      }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), 13 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return 0;
}
