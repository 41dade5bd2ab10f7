// host_plan_chance_sampled.cpp — the host form of cilqr_chance_risk_sampled in the arena: plain C++ over csrc/cilqr_host_plan.h, no HIP.
//   1. Over a grid of small shapes plan_chance_sampled is laid out without an arena and its declared arrays are checked one by one:
//      their number, order, sizes, 16-byte-aligned offsets, the contiguous input prefix [0, in_end) and output suffix
//      [out_begin, end), with every optional output present or absent.
//   2. For every (max_batch, max_horizon, max_obstacles) triple on the command line it prints host_arena_bytes — the test compares
//      it with tests/golden/host_arena_cap.json: the arena is the one the earlier calls sized — and checks what include/cilqr.h
//      says always fits against it, at N = max_horizon and n_obs*n_samples = max_obstacles for the two extreme splits (one
//      obstacle, and two samples per obstacle): without entry_p every B <= max_batch; with it every B <= max_batch where
//      max_horizon >= 2, and every B <= max_batch / 2 where max_horizon = 1.
// Prints "layout ok" and "every shape fits"; exit code 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "cilqr_host_plan.h"

static double host;

struct Plan {
  cilqr::HostPlan p{nullptr};
  Plan(size_t B, size_t N, size_t n_obs, size_t ns, bool base_total, bool step, bool pair, bool entry) {
    const double *X = &host, *sigma = &host, *np = &host, *nd = &host, *off = &host, *base = base_total ? &host : nullptr;
    double *risk = &host, *sr = step ? &host : nullptr, *pp = pair ? &host : nullptr, *ep = entry ? &host : nullptr;
    double* total = base_total ? &host : nullptr;
    cilqr::plan_chance_sampled(p, B, N, n_obs, ns, X, sigma, np, nd, off, base, risk, sr, pp, ep, total);
  }
};

static int check_layout() {
  int bad = 0, n = 0;
  const size_t Bs[] = {1, 2, 3, 7}, Ns[] = {1, 2, 5, 12}, Os[] = {1, 2, 3}, Ss[] = {2, 5, 32};
  for (size_t B : Bs)
    for (size_t N : Ns)
      for (size_t n_obs : Os)
        for (size_t ns : Ss)
          for (int mask = 0; mask < 16; ++mask) {
            const bool bt = mask & 1, step = mask & 2, pair = mask & 4, entry = mask & 8;
            Plan pl(B, N, n_obs, ns, bt, step, pair, entry);
            const cilqr::HostPlan& p = pl.p;
            // the arrays in declaration order: doubles each, travels in (1) or out (0); 0 doubles: not declared
            const size_t want[11][2] = {{B * 4 * (N + 1), 1}, {B * (N + 1) * 16, 1}, {B * n_obs * N * 4, 1}, {B * n_obs * N * 2, 1},
                                        {B * n_obs * ns * 3, 1}, {bt ? B : 0, 1}, {B * CILQR_CRS_FIELDS, 0}, {step ? B * N : 0, 0},
                                        {pair ? B * n_obs * N : 0, 0}, {entry ? B * n_obs * ns * N : 0, 0}, {bt ? B : 0, 0}};
            size_t at = 0, in_end = 0;
            int k = 0;
            bool ok = p.ok;
            for (int i = 0; i < 11 && ok; ++i) {
              if (!want[i][0]) continue;
              const cilqr::HostPlan::Entry& e = p.e[k++];
              ok = k <= p.n && e.off == at && e.off % 16 == 0 && e.bytes == want[i][0] * sizeof(double) &&
                   (want[i][1] ? e.src && !e.dst : !e.src && e.dst);
              at = (at + e.bytes + 15) & ~(size_t)15;
              if (want[i][1]) in_end = at;
            }
            ok = ok && k == p.n && p.end == at && p.in_end == in_end && p.out_begin == in_end;
            ++n;
            if (!ok) {
              printf("B %zu N %zu n_obs %zu n_samples %zu outputs %d: layout differs (%d arrays, end %zu)\n", B, N, n_obs, ns, mask, p.n, p.end);
              ++bad;
            }
          }
  if (!bad) printf("layout ok (%d plans), 11 arrays at most of %d\n", n, (int)cilqr::HostPlan::CAP);
  return bad;
}

int main(int argc, char** argv) {
  int bad = check_layout(), n = 0;
  for (int i = 1; i + 2 < argc; i += 3) {
    const size_t B = strtoul(argv[i], nullptr, 10), N = strtoul(argv[i + 1], nullptr, 10), M = strtoul(argv[i + 2], nullptr, 10);
    const size_t cap = cilqr::host_arena_bytes(B, N, M);
    printf("arena %zu %zu %zu = %zu\n", B, N, M, cap);
    if (M < 2) continue;  // (no sampled scene fits such a handle: n_samples >= 2)
    const size_t splits[2][2] = {{1, M}, {M / 2, 2}};  // (n_obs, n_samples)
    for (const auto& s : splits) {
      const size_t lean = Plan(B, N, s[0], s[1], true, true, true, false).p.end;
      const size_t Bf = N >= 2 ? B : B / 2;
      const size_t full = Bf ? Plan(Bf, N, s[0], s[1], true, true, true, true).p.end : 0;
      const bool fits = lean <= cap && full <= cap;
      n += 2;
      if (!fits || (B == 64 && N == 50)) {
        printf("max_batch %zu N %zu, %zu x %zu samples: without entry_p at B %zu %zu bytes, with it at B %zu %zu bytes, arena %zu%s\n", B, N,
               s[0], s[1], B, lean, Bf, full, cap, fits ? "" : "  DOES NOT FIT");
      }
      bad += !fits;
    }
  }
  if (bad) { printf("%d failures\n", bad); return 1; }
  printf("every shape fits (%d shapes)\n", n);
  return 0;
}
