// host_plan_track_map.cpp — does the host form of cilqr_rasterize_tracks fit the arena cilqr_create reserves, at the shape
// include/cilqr.h says always fits, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h,
// no HIP: plan_rasterize_tracks is laid out without an arena (sizes and offsets only) for the node's 150 x 100 map at N = 50 with
// one shared set of 8 tracks,
//   - with X and obs_cov at B = max_batch/8 on handles of max_batch >= 8, max_horizon >= 50, max_obstacles >= 8,
//   - swept (no X) and without obs_cov at the same B,
// and its end is compared with host_arena_bytes(max_batch, max_horizon, max_obstacles); the plan at B = max_batch is reported (it
// need not fit: the call then returns CILQR_ERR_ARG).  For every (B, N, M) triple on the command line it prints host_arena_bytes,
// which the test compares with tests/golden/host_arena_cap.json: the arena is the one the earlier calls sized.
// Prints one line per reported shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static size_t plan_end(size_t B, size_t N, size_t M, size_t cells, bool all, int* n_arrays, bool* ok) {
  static double host;
  static float layer;
  const double *X = all ? &host : nullptr, *cov = all ? &host : nullptr;
  float* out = &layer;
  double* fields = &host;
  cilqr_obstacles o = {&host, &host, &host, 0, (int64_t)N, 1, 0};
  cilqr::HostPlan p(nullptr);
  cilqr::plan_rasterize_tracks(p, B, N, cells, X, o, M * N, cov, out, fields);
  *n_arrays = p.n;
  *ok = p.ok;
  return p.end;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t cells = 150 * 100, N = 50, M = 8;
  const size_t batches[] = {8, 9, 15, 16, 64, 1000, 1024, 4096}, horizons[] = {50, 51, 383, CILQR_MAX_HORIZON}, obstacles[] = {8, 9, 64};
  int bad = 0, n = 0;
  for (size_t mb : batches)
    for (size_t mh : horizons)
      for (size_t mo : obstacles) {
        const size_t cap = cilqr::host_arena_bytes(mb, mh, mo), B = mb / 8;
        const bool show = mb == 1024 && mh == 50 && mo == 8;
        for (int all = 0; all < 2; ++all) {
          int arrays = 0;
          bool ok = false;
          const size_t end = plan_end(B, N, M, cells, all != 0, &arrays, &ok);
          const bool fits = ok && arrays == (all ? 6 : 4) && end <= cap;
          ++n;
          if (!fits || show)
            printf("B %zu of max_batch %zu, max_horizon %zu, max_obstacles %zu, %s: plan %zu of %zu bytes, %d arrays%s\n", B, mb, mh, mo,
                   all ? "X and obs_cov" : "swept, no obs_cov", end, cap, arrays, fits ? "" : "  DOES NOT FIT");
          bad += !fits;
        }
        if (show) {
          int arrays = 0;
          bool ok = false;
          const size_t full = plan_end(mb, N, M, cells, true, &arrays, &ok);
          printf("B %zu, X and obs_cov: plan %zu of %zu bytes (%s)\n", mb, full, cap, full <= cap ? "fits" : "CILQR_ERR_ARG");
        }
      }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), 6 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return 0;
}
