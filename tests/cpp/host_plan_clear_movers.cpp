// host_plan_clear_movers.cpp — does the host form of cilqr_clear_movers fit the arena cilqr_create reserves at the node's shape, and
// is that arena still the one the earlier calls sized?  Plain C++ over csrc/cilqr_host_plan.h, no HIP.  plan_clear_movers is laid
// out without an arena (sizes and offsets only) in its two mover forms, with and without owner_out, for one 150 x 100 layer with
// K = 8 rows and M = 8 slots, and its end is compared with host_arena_bytes of the node's handle (max_batch 1024, max_horizon 50,
// max_obstacles 4); then for L = 16 layers, which fit as well, and for L = 1024, which do not (the call then returns CILQR_ERR_ARG:
// large batches take the device form).  For every (B, N, M) triple on the command line it prints host_arena_bytes, which the test
// compares with tests/golden/host_arena_cap.json.
// Prints the layouts and "the node's shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static cilqr::HostPlan lay(size_t L, size_t cells, size_t K, size_t M, bool tracker, bool with_owner) {
  static float fhost[2];
  static double host[2];
  static int32_t ihost[2];
  const float* layer = fhost;
  const int32_t *label = ihost, *assign = tracker ? ihost : nullptr, *mask = tracker ? nullptr : ihost;
  const double *comp = host, *state = tracker ? host : nullptr;
  float* layer_out = fhost;
  int32_t* owner = with_owner ? ihost : nullptr;
  double* fields = host;
  cilqr::HostPlan p(nullptr);
  cilqr::plan_clear_movers(p, L, cells, L * cells, K, tracker ? M : 0, layer, label, comp, assign, state, mask, layer_out, owner, fields);
  return p;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cilqr::host_arena_bytes(B, N, M));
  }
  const size_t cells = 150 * 100, K = 8, M = 8, cap = cilqr::host_arena_bytes(1024, 50, 4);
  int bad = 0, most = 0;
  for (int tracker = 1; tracker >= 0; --tracker)
    for (int owner = 1; owner >= 0; --owner) {
      const cilqr::HostPlan p = lay(1, cells, K, M, tracker != 0, owner != 0);
      const int expect = (tracker ? 5 : 4) + (owner ? 3 : 2);
      if (p.n > most) most = p.n;
      bad += !(p.ok && p.n == expect && p.end <= cap);
      if (tracker == owner)
        printf("layout %s: %d arrays, in_end %zu, out_begin %zu, end %zu\n", tracker ? "tracker" : "mask, no owner", p.n, p.in_end, p.out_begin, p.end);
    }
  const cilqr::HostPlan p16 = lay(16, cells, K, M, true, true), p1024 = lay(1024, cells, K, M, true, true);
  printf("L 16: plan %zu of %zu bytes; L 1024: plan %zu bytes%s\n", p16.end, cap, p1024.end, p1024.end > cap ? " (beyond the arena: CILQR_ERR_ARG)" : "");
  bad += !(p16.ok && p16.end <= cap) + !(p1024.ok && p1024.end > cap);
  if (bad) { printf("%d layouts are not what they should be\n", bad); return 1; }
  printf("the node's shape fits (%zu of %zu bytes), %d arrays at most of %d\n", lay(1, cells, K, M, true, true).end, cap, most, (int)cilqr::HostPlan::CAP);
  return 0;
}
