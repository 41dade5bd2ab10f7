// host_plan_footprint.cpp — does the host form of cilqr_footprint_check fit the arena cilqr_create reserves at every shape
// include/cilqr.h says fits, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h, no
// HIP: plan_footprint is laid out without an arena (sizes and offsets only) at R = B*S = max_batch rows, N = max_horizon, dense
// obstacles (span B*M*N) and one static set (span M), with every output and with fp alone, and its end is compared with
// host_arena_bytes(max_batch, max_horizon, max_obstacles).  For every (B, N, M) triple on the command line it prints
// host_arena_bytes, which the test compares with tests/golden/host_arena_cap.json; with "layout R N M span all" it prints one plan's
// entries as "entry off bytes in out".  Prints "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cilqr_host_plan.h"

static cilqr::HostPlan lay(size_t R, size_t N, size_t M, size_t span, bool all) {
  static double host;
  static float hostf;
  const double *X = &host, *base = all ? &host : nullptr;
  double *fp = &host, *sc = all ? &host : nullptr, *total = all ? &host : nullptr;
  float* so = all ? &hostf : nullptr;
  cilqr_obstacles o = {&host, &host, &host, 0, 0, 0, 0};
  cilqr::HostPlan p(nullptr);
  cilqr::plan_footprint(p, R, N, M, X, o, span, base, fp, sc, so, total);
  return p;
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "layout")) {
    const size_t R = strtoul(argv[2], nullptr, 10), N = strtoul(argv[3], nullptr, 10), M = strtoul(argv[4], nullptr, 10);
    const cilqr::HostPlan p = lay(R, N, M, strtoul(argv[5], nullptr, 10), atoi(argv[6]) != 0);
    for (int i = 0; i < p.n; ++i) printf("entry %zu %zu %d %d\n", p.e[i].off, p.e[i].bytes, p.e[i].src ? 1 : 0, p.e[i].dst ? 1 : 0);
    printf("plan ok %d in_end %zu out_begin %zu end %zu\n", p.ok ? 1 : 0, p.in_end, p.out_begin, p.end);
    return 0;
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 6, 16, 64, 1024, 4096}, horizons[] = {1, 5, 50, CILQR_MAX_HORIZON}, obstacles[] = {0, 1, 4, 70};
  int bad = 0, n = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles)
        for (int dense = 0; dense < 2; ++dense)
          for (int all = 0; all < 2; ++all) {
            const size_t cap = cilqr::host_arena_bytes(B, N, M);
            const cilqr::HostPlan p = lay(B, N, M, dense ? B * M * N : M, all != 0);  // (S = 1: B solves are B rows; S > 1 has fewer solves)
            const int want = (M ? 2 : 0) + (all ? 6 : 2);
            const bool fits = p.ok && p.n == want && p.end <= cap;
            ++n;
            if (!fits || (B == 16 && N == 50 && M == 4))
              printf("R %zu N %zu M %zu %s, %s: plan %zu of %zu bytes, %d arrays%s\n", B, N, M, dense ? "dense" : "static", all ? "every output" : "fp alone",
                     p.end, cap, p.n, fits ? "" : "  DOES NOT FIT");
            bad += !fits;
          }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), 8 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return 0;
}
