// host_plan_chance_map.cpp — does the host form of cilqr_chance_risk_map fit the arena cilqr_create reserves, at the shapes
// include/cilqr.h says always fit, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h,
// no HIP: plan_chance_risk_map is laid out without an arena (sizes and offsets only) with Q = 1, 75 and CILQR_MAX_QUAD_NODES nodes,
//   - without per-step outputs at B = max_batch, N = max_horizon, wherever 4*Q <= max_batch*(2*max_horizon + 4),
//   - with the three per-step outputs at B = 7*max_batch/8, wherever 4*Q <= max_batch*(max_horizon + 7),
// and its end is compared with host_arena_bytes(max_batch, max_horizon, max_obstacles).  For every (B, N, M) triple on the command
// line it prints host_arena_bytes, which the test compares with tests/golden/host_arena_cap.json.  Prints one line per reported
// shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static size_t plan_end(size_t B, size_t N, size_t Q, bool steps, int* n_arrays, bool* ok) {
  static double host;
  const double *X = &host, *sigma = &host, *nodes = &host, *weights = &host, *base = &host;
  double *risk = &host, *total = &host;
  double *sr = steps ? &host : nullptr, *so = steps ? &host : nullptr, *su = steps ? &host : nullptr;
  cilqr::HostPlan p(nullptr);
  cilqr::plan_chance_risk_map(p, B, N, Q, X, sigma, nodes, weights, base, risk, sr, so, su, total);
  *n_arrays = p.n;
  *ok = p.ok;
  return p.end;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 8, 15, 16, 64, 1024, 4096}, horizons[] = {1, 2, 12, 50, 383, CILQR_MAX_HORIZON}, obstacles[] = {0, 4};
  const size_t quads[] = {1, 75, CILQR_MAX_QUAD_NODES};
  int bad = 0, n = 0, skipped = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles)
        for (size_t Q : quads) {
          const size_t cap = cilqr::host_arena_bytes(B, N, M);
          const bool show = B == 16 && N == 50 && M == 0;
          int arrays = 0;
          bool ok = false;
          if (4 * Q <= B * (2 * N + 4)) {
            const size_t lean = plan_end(B, N, Q, false, &arrays, &ok);
            const bool fits = ok && arrays == 7 && lean <= cap;
            ++n;
            if (!fits || show) printf("B %zu N %zu M %zu Q %zu, no per-step output: plan %zu of %zu bytes, %d arrays%s\n", B, N, M, Q, lean, cap, arrays, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          } else {
            ++skipped;
          }
          const size_t Bs = 7 * B / 8;
          if (Bs >= 1 && 4 * Q <= B * (N + 7)) {
            const size_t full = plan_end(Bs, N, Q, true, &arrays, &ok);
            const bool fits = ok && arrays == 10 && full <= cap;
            ++n;
            if (!fits || show) printf("B %zu of max_batch %zu, N %zu M %zu Q %zu, every output: plan %zu of %zu bytes, %d arrays%s\n", Bs, B, N, M, Q, full, cap, arrays, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          } else {
            ++skipped;
          }
        }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes, %d outside the promise), 10 arrays at most of %d\n", n, skipped, (int)cilqr::HostPlan::CAP);
  return 0;
}
