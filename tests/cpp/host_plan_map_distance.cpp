// host_plan_map_distance.cpp — do the host forms of cilqr_map_distance, cilqr_inflate_map and cilqr_map_clearance fit the arena
// cilqr_create reserves, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h, no HIP.
//   * for every (B, N, M) triple on the command line it prints host_arena_bytes, which the test compares with
//     tests/golden/host_arena_cap.json;
//   * plan_map_clearance is laid out without an arena at R = B*S = max_batch rows and N = max_horizon, with every output and with
//     mc alone, and its end is compared with host_arena_bytes(max_batch, max_horizon, max_obstacles): "every clearance shape fits";
//   * with "layers L cells span dist" it prints the entries of plan_map_distance ("distance ...") and of plan_inflate_map
//     ("inflate ...") as "entry off bytes in out" and each plan's end: the arena is sized by the solves, not by maps, so whether
//     a map call fits is the transport's comparison of that end with the arena (the test takes both sides of it).
// Exit code 1 when a clearance shape does not fit.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cilqr_host_plan.h"

static void print(const char* name, const cilqr::HostPlan& p) {
  for (int i = 0; i < p.n; ++i) printf("%s entry %zu %zu %d %d\n", name, p.e[i].off, p.e[i].bytes, p.e[i].src ? 1 : 0, p.e[i].dst ? 1 : 0);
  printf("%s plan ok %d in_end %zu out_begin %zu end %zu\n", name, p.ok ? 1 : 0, p.in_end, p.out_begin, p.end);
}

int main(int argc, char** argv) {
  static double host;
  static float hostf;
  static int32_t hosti;
  if (argc == 6 && !strcmp(argv[1], "layers")) {
    const size_t L = strtoul(argv[2], nullptr, 10), cells = strtoul(argv[3], nullptr, 10), span = strtoul(argv[4], nullptr, 10);
    {
      const float* layer = &hostf;
      int32_t* d2 = &hosti;
      float* dist = atoi(argv[5]) ? &hostf : nullptr;
      cilqr::HostPlan p(nullptr);
      cilqr::plan_map_distance(p, L, cells, span, layer, d2, dist);
      print("distance", p);
    }
    {
      const float* layer = &hostf;
      const int32_t* d2 = &hosti;
      float* out = &hostf;
      cilqr::HostPlan p(nullptr);
      cilqr::plan_inflate_map(p, L, cells, span, layer, d2, out);
      print("inflate", p);
    }
    return 0;
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 6, 16, 64, 1024, 4096}, horizons[] = {1, 5, 50, CILQR_MAX_HORIZON}, obstacles[] = {0, 4};
  int bad = 0, n = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles)
        for (int all = 0; all < 2; ++all) {
          const double *X = &host, *base = all ? &host : nullptr;
          double *mc = &host, *sc = all ? &host : nullptr, *total = all ? &host : nullptr;
          cilqr::HostPlan p(nullptr);
          cilqr::plan_map_clearance(p, B, N, X, base, mc, sc, total);
          const size_t cap = cilqr::host_arena_bytes(B, N, M);
          const bool fits = p.ok && p.n == (all ? 5 : 2) && p.end <= cap;
          ++n;
          if (!fits || (B == 16 && N == 50 && M == 0))
            printf("R %zu N %zu M %zu, %s: plan %zu of %zu bytes, %d arrays%s\n", B, N, M, all ? "every output" : "mc alone", p.end, cap, p.n,
                   fits ? "" : "  DOES NOT FIT");
          bad += !fits;
        }
  if (bad) { printf("%d of %d clearance shapes do not fit\n", bad, n); return 1; }
  printf("every clearance shape fits (%d shapes), 5 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return 0;
}
