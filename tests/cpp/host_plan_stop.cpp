// host_plan_stop.cpp — does the host form of cilqr_stop_plans fit the arena cilqr_create reserves at every shape include/cilqr.h says
// fits, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h, no HIP: plan_stop_plans is
// laid out without an arena (sizes and offsets only) at B*D = max_batch rows in every split of max_batch into plans and levels,
// N = max_horizon, with every output and with the required ones alone, and its end is compared with host_arena_bytes(max_batch,
// max_horizon, max_obstacles).  For every (B, N, M) triple on the command line it prints host_arena_bytes, which the test compares
// with tests/golden/host_arena_cap.json; with "layout B N D all" it prints one plan's entries as "entry off bytes in out".  Prints
// "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cilqr_host_plan.h"

static cilqr::HostPlan lay(size_t B, size_t N, size_t D, bool all) {
  static double host;
  const double *X = &host, *U = &host, *decel = &host, *plan_cost = all ? &host : nullptr;
  double *Xs = &host, *Us = &host, *sp = &host, *cost = all ? &host : nullptr;
  cilqr::HostPlan p(nullptr);
  cilqr::plan_stop_plans(p, B, N, D, X, U, decel, plan_cost, Xs, Us, sp, cost);
  return p;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "layout")) {
    const size_t B = strtoul(argv[2], nullptr, 10), N = strtoul(argv[3], nullptr, 10), D = strtoul(argv[4], nullptr, 10);
    const cilqr::HostPlan p = lay(B, N, D, atoi(argv[5]) != 0);
    for (int i = 0; i < p.n; ++i) printf("entry %zu %zu %d %d\n", p.e[i].off, p.e[i].bytes, p.e[i].src ? 1 : 0, p.e[i].dst ? 1 : 0);
    printf("plan ok %d in_end %zu out_begin %zu end %zu\n", p.ok ? 1 : 0, p.in_end, p.out_begin, p.end);
    return 0;
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 6, 16, 64, 1024, 4096}, horizons[] = {1, 5, 50, CILQR_MAX_HORIZON}, obstacles[] = {0, 4};
  int bad = 0, n = 0;
  for (size_t R : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles)
        for (size_t D = 1; D <= R; ++D) {  // every split of max_batch rows into plans and levels that uses all of them
          if (R % D) continue;
          for (int all = 0; all < 2; ++all) {
            const size_t cap = cilqr::host_arena_bytes(R, N, M);
            const cilqr::HostPlan p = lay(R / D, N, D, all != 0);
            const bool fits = p.ok && p.n == (all ? 8 : 6) && p.end <= cap;
            ++n;
            if (!fits || (R == 16 && N == 50 && M == 4 && D == 4))
              printf("B %zu D %zu N %zu M %zu, %s: plan %zu of %zu bytes, %d arrays%s\n", R / D, D, N, M, all ? "every array" : "required arrays alone",
                     p.end, cap, p.n, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          }
        }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), 8 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return 0;
}
