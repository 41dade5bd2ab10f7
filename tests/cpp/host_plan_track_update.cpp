// host_plan_track_update.cpp — does the host form of cilqr_track_update fit the arena cilqr_create reserves at the shapes
// include/cilqr.h says always fit, and is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h,
// no HIP.  plan_track_update is laid out without an arena (sizes and offsets only) in its three forms — in place, with a separate
// state_out, under CILQR_TRACK_RESET — at W = max_batch, M = min(max_obstacles, 64), D = 64, one count per world, on every handle
// with max_horizon >= 15, and each end is compared with host_arena_bytes(max_batch, max_horizon, max_obstacles).  Shorter horizons
// are reported (they need not fit: the call then returns CILQR_ERR_ARG).  The plan's own layout is printed for one shape: which
// arrays travel in, which back, and that an in-place state is one array.  For every (B, N, M) triple on the command line it prints
// host_arena_bytes, which the test compares with tests/golden/host_arena_cap.json.
// Prints one line per reported shape and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

enum Form { IN_PLACE, SEPARATE, RESET };

static size_t track_end(size_t W, size_t M, size_t D, Form form, bool counts, bool with_assign, cilqr::HostPlan* keep, bool* same_state) {
  static double host[2];
  static int32_t ihost[2];
  const double* det = D ? host : nullptr;
  const int32_t* n_det = counts ? ihost : nullptr;
  const double* state_in = form == RESET ? nullptr : host;
  double* state_out = form == SEPARATE ? host + 1 : host;
  double *world = host, *track = host, *dim = host, *cov = host;
  int32_t* assign = with_assign && D ? ihost : nullptr;
  cilqr::HostPlan p(nullptr);
  cilqr::plan_track_update(p, W, M, D, counts ? W : 0, form == RESET, det, n_det, state_in, state_out, world, assign, track, dim, cov);
  *same_state = state_in == state_out;
  if (keep) *keep = p;
  return p.ok ? p.end : (size_t)-1;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t batches[] = {1, 2, 3, 5, 8, 15, 16, 64, 1024, 4096}, horizons[] = {1, 2, 12, 14, 15, 50, 383, CILQR_MAX_HORIZON}, obstacles[] = {1, 4, 63, 64, 1024};
  const char* names[] = {"in place", "separate state_out", "reset"};
  int bad = 0, n = 0, most = 0, short_misfits = 0;
  for (size_t B : batches)
    for (size_t N : horizons)
      for (size_t Mh : obstacles) {
        const size_t cap = cilqr::host_arena_bytes(B, N, Mh), M = Mh < CILQR_TRACK_MAX_SLOTS ? Mh : CILQR_TRACK_MAX_SLOTS, D = CILQR_TRACK_MAX_DETECTIONS;
        for (int form = 0; form < 3; ++form) {
          cilqr::HostPlan p(nullptr);
          bool same = false;
          const size_t end = track_end(B, M, D, (Form)form, true, true, &p, &same);
          const int expect = form == SEPARATE ? 9 : 8;
          // bytes the formula of the header gives: W*(56*M + 5.5*D + 9) doubles in place, 32*W*M more when separate, and the counts
          const size_t formula = 8 * B * (56 * M + 5 * D + 9) + 4 * B * D + (form == SEPARATE ? 8 * 32 * B * M : 0) + 4 * B;
          const bool shape_ok = end != (size_t)-1 && p.n == expect && end >= formula && end <= formula + 16 * (size_t)expect;  // (an in-place state is one array: 8 against 9)
          if (p.n > most) most = p.n;
          const bool show = B == 1024 && N == 50 && Mh == 4;
          if (N >= 15) {
            const bool fits = shape_ok && end <= cap;
            ++n;
            bad += !fits;
            if (!fits || show) printf("track_update W %zu N %zu M %zu D %zu, %s: plan %zu of %zu bytes, %d arrays%s\n", B, N, M, D, names[form], end, cap, p.n, fits ? "" : "  DOES NOT FIT");
          } else {
            bad += !shape_ok;
            if (end > cap) ++short_misfits;
          }
        }
      }
  {
    // the layout of one call: W 2, M 4, D 3, in place with counts and assign
    cilqr::HostPlan p(nullptr);
    bool same = false;
    track_end(2, 4, 3, IN_PLACE, true, true, &p, &same);
    printf("layout in place: %d arrays, in_end %zu, out_begin %zu, end %zu\n", p.n, p.in_end, p.out_begin, p.end);
    for (int i = 0; i < p.n; ++i) printf("  array %d: off %zu bytes %zu %s%s\n", i, p.e[i].off, p.e[i].bytes, p.e[i].src ? "in" : "", p.e[i].dst ? "out" : "");
    cilqr::HostPlan q(nullptr);
    track_end(2, 4, 0, RESET, false, true, &q, &same);
    printf("layout reset, D 0: %d arrays, in_end %zu, out_begin %zu, end %zu\n", q.n, q.in_end, q.out_begin, q.end);
  }
  printf("horizons below 15: %d of the plans exceed their arena (CILQR_ERR_ARG)\n", short_misfits);
  if (bad) { printf("%d of %d shapes do not fit\n", bad, n); return 1; }
  printf("every shape fits (%d shapes), %d arrays at most of %d\n", n, most, (int)cilqr::HostPlan::CAP);
  return 0;
}
