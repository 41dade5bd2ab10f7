// host_plan_risk_map.cpp — does the host form of cilqr_rollout_risk_map fit the arena cilqr_create reserves, at the shapes
// include/cilqr.h says always fit?  Plain C++ over csrc/cilqr_host_plan.h, no HIP: plan_rollout_risk_map is laid out without an
// arena (sizes and offsets only) at B = max_batch, N = max_horizon and (delta_batch_stride ? B : 1)*S = max_batch*max_horizon,
// for shared and per-solve offsets and every output asked for, and its end is compared with host_arena_bytes(max_batch,
// max_horizon, max_obstacles).  Prints one line per shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>

#include "cilqr_host_plan.h"

int main() {
  static double host;
  static int32_t ihost;
  const size_t batches[] = {1, 2, 15, 16, 64, 1024, 4096}, horizons[] = {1, 2, 12, 50, 383, CILQR_MAX_HORIZON}, obstacles[] = {0, 4};
  int bad = 0, n = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles)
        for (int per_solve = 0; per_solve < 2; ++per_solve) {
          // the most offsets the header promises: (per_solve ? B : 1)*S = B*N, S whole
          const size_t sets = per_solve ? B : 1, S = B * N / sets;
          const double *X = &host, *U = &host, *k = &host, *K = &host, *delta = &host, *base = &host;
          double *risk = &host, *total = &host;
          int32_t *hits = &ihost, *unknown = &ihost;
          cilqr::HostPlan p(nullptr);
          cilqr::plan_rollout_risk_map(p, B, N, S, sets, X, U, k, K, delta, base, risk, hits, unknown, total);
          const size_t cap = cilqr::host_arena_bytes(B, N, M);
          const bool fits = p.ok && p.n == 10 && p.end <= cap;
          ++n;
          if (!fits || (B == 1024 && N == 50)) printf("B %zu N %zu M %zu S %zu x %zu sets: plan %zu of %zu bytes, %d arrays%s\n", B, N, M, S, sets, p.end, cap, p.n, fits ? "" : "  DOES NOT FIT");
          bad += !fits;
        }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes)\n", n);
  return 0;
}
