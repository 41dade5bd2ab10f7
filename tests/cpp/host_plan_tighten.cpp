// host_plan_tighten.cpp — does the host form of cilqr_tighten_obstacles fit the arena cilqr_create reserves, at the shapes
// include/cilqr.h says always fit, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h,
// no HIP: plan_tighten_obstacles is laid out without an arena (sizes and offsets only) with dense obstacles,
//   - with obs_cov and pose_out at B = 2*max_batch/5, N = max_horizon, M = max_obstacles,
//   - without the two at B = 3*max_batch/4,
//   - with M = 0 at B = max_batch,
// and its end is compared with host_arena_bytes(max_batch, max_horizon, max_obstacles); the plan with everything at B = max_batch is
// reported (it need not fit: the call then returns CILQR_ERR_ARG).  For every (B, N, M) triple on the command line it prints
// host_arena_bytes, which the test compares with tests/golden/host_arena_cap.json: the arena is the one the earlier calls sized.
// Prints one line per reported shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static size_t plan_end(size_t B, size_t N, size_t M, bool all, int* n_arrays, bool* ok) {
  static double host;
  const double *X = &host, *sigma = &host, *cov = all ? &host : nullptr;
  double *pose = all ? &host : nullptr, *dim = &host, *tg = &host;
  cilqr_obstacles o = {&host, &host, &host, 0, 0, 0, 0};
  cilqr::HostPlan p(nullptr);
  cilqr::plan_tighten_obstacles(p, B, N, M, X, sigma, o, B * M * N, cov, pose, dim, tg);
  *n_arrays = p.n;
  *ok = p.ok;
  return p.end;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 5, 15, 16, 64, 1024, 4096}, horizons[] = {1, 2, 12, 50, 383, CILQR_MAX_HORIZON}, obstacles[] = {0, 1, 4, 64};
  int bad = 0, n = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t M : obstacles) {
        const size_t cap = cilqr::host_arena_bytes(B, N, M);
        const bool show = B == 1024 && N == 50 && M == 4;
        int arrays = 0;
        bool ok = false;
        if (M == 0) {
          const size_t end = plan_end(B, N, 0, true, &arrays, &ok);
          const bool fits = ok && arrays == 3 && end <= cap;  // X, sigma, tighten: nothing else has a place
          ++n;
          if (!fits) printf("B %zu N %zu M 0: plan %zu of %zu bytes, %d arrays  DOES NOT FIT\n", B, N, end, cap, arrays);
          bad += !fits;
          continue;
        }
        if (2 * B / 5 >= 1) {
          const size_t Bq = 2 * B / 5, end = plan_end(Bq, N, M, true, &arrays, &ok);
          const bool fits = ok && arrays == 8 && end <= cap;
          ++n;
          if (!fits || show) printf("B %zu of max_batch %zu, N %zu M %zu, obs_cov and pose_out: plan %zu of %zu bytes, %d arrays%s\n", Bq, B, N, M, end, cap, arrays, fits ? "" : "  DOES NOT FIT");
          bad += !fits;
        }
        if (3 * B / 4 >= 1) {
          const size_t Bq = 3 * B / 4, end = plan_end(Bq, N, M, false, &arrays, &ok);
          const bool fits = ok && arrays == 6 && end <= cap;
          ++n;
          if (!fits || show) printf("B %zu of max_batch %zu, N %zu M %zu, neither: plan %zu of %zu bytes, %d arrays%s\n", Bq, B, N, M, end, cap, arrays, fits ? "" : "  DOES NOT FIT");
          bad += !fits;
        }
        const size_t full = plan_end(B, N, M, true, &arrays, &ok);
        if (show) printf("B %zu N %zu M %zu, obs_cov and pose_out: plan %zu of %zu bytes (%s)\n", B, N, M, full, cap, full <= cap ? "fits" : "CILQR_ERR_ARG");
      }
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), 8 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return 0;
}
