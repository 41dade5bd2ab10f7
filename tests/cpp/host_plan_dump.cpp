// host_plan_dump.cpp — prints where the arrays of a host-buffer call lie in the device arena (csrc/cilqr_host_plan.h), one JSON
// line per shape on the command line, and the arena a handle of max_B / max_N / max_M reserves (all a shape without a form prints).  No GPU, no HIP:
// tests/test_host_plan.py.  A shape is "form=NAME,name=value,…" over B N M S n_samples span w_span delta_sets and the switches
// weights (obstacle weights given), opt (optional outputs and `base` given); NAME is the C-ABI call without its cilqr_ prefix (or one of two malformed plans).
// Each entry prints as [offset, bytes, travels in, travels back]; "at" gives the offset each pointer was swapped for (-1: null).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cilqr_host_plan.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    long B = 0, N = 1, M = 0, S = 1, n_samples = 0, span = 0, w_span = 0, delta_sets = 1, weights = 0, opt = 0, max_B = 1, max_N = 1, max_M = 0;
    std::string form;
    const struct { const char* name; long* v; } fields[] = {
        {"B", &B}, {"N", &N}, {"M", &M}, {"S", &S}, {"n_samples", &n_samples}, {"span", &span}, {"w_span", &w_span}, {"delta_sets", &delta_sets},
        {"weights", &weights}, {"opt", &opt}, {"max_B", &max_B}, {"max_N", &max_N}, {"max_M", &max_M}};
    for (char* tok = strtok(argv[i], ","); tok; tok = strtok(nullptr, ",")) {
      char* eq = strchr(tok, '=');
      bool known = eq && strncmp(tok, "form=", 5) == 0;
      if (known) form = eq + 1;
      for (const auto& f : fields)
        if (eq && strlen(f.name) == (size_t)(eq - tok) && strncmp(f.name, tok, eq - tok) == 0) { *f.v = atol(eq + 1); known = true; }
      if (!known) { fprintf(stderr, "host_plan_dump: bad field '%s'\n", tok); return 2; }
    }
    const size_t cap = cilqr::host_arena_bytes(max_B, max_N, max_M);
    if (form.empty()) { printf("{\"cap\": %zu}\n", cap); continue; }  // the arena alone
    std::vector<char> arena(cap + 16);
    char* base = arena.data();
    // host pointers to declare with: never read, told apart from the arena by their addresses
    static double host_d[4];
    static int32_t host_i[4];
    const double *a = host_d, *b = host_d, *c = host_d, *d = host_d, *e = host_d, *base_cost = opt ? host_d : nullptr, *samp = n_samples ? host_d : nullptr;
    double *u = host_d, *x = host_d, *y = host_d, *z = opt ? host_d : nullptr;
    int32_t *it = opt ? host_i : nullptr, *st = opt ? host_i : nullptr;
    cilqr_obstacles o = {host_d, host_d, weights ? host_d : nullptr, 0, 0, 0, 0};
    cilqr::HostPlan p(base);
    std::vector<std::pair<const char*, const void*>> at;
    if (form == "solve_batch" || form == "solve_batch_obstacles" || form == "solve_batch_sampled") {
      cilqr::plan_solve(p, B, N, M, n_samples, a, u, b, c, o, span, w_span, samp, x, z, it, st);
      at = {{"x0", a}, {"U", u}, {"poly", b}, {"xplan_fl", c}, {"samp_off", samp}, {"X_out", x}, {"J_out", z}, {"iters_out", it}, {"status_out", st}};
    } else if (form == "score_batch" || form == "score_batch_sampled") {
      cilqr::plan_score(p, B, N, M, n_samples, a, b, c, d, o, span, w_span, samp, x, z);
      at = {{"X", a}, {"U", b}, {"poly", c}, {"xplan_fl", d}, {"samp_off", samp}, {"score", x}, {"total", z}};
    } else if (form == "gains_batch") {
      cilqr::plan_gains(p, B, N, M, a, b, c, d, o, span, w_span, x, y, it);
      at = {{"X", a}, {"U", b}, {"poly", c}, {"xplan_fl", d}, {"k_out", x}, {"K_out", y}, {"ok_out", it}};
    } else if (form == "rollout_batch") {
      cilqr::plan_rollout(p, B, N, S, delta_sets, a, b, c, d, e, x, y);
      at = {{"X", a}, {"U", b}, {"k", c}, {"K", d}, {"delta", e}, {"X_roll", x}, {"U_roll", y}};
    } else if (form == "score_rollouts") {
      cilqr::plan_score_rollouts(p, B, N, M, S, a, b, c, d, o, span, w_span, x, y, z);
      at = {{"X_roll", a}, {"U_roll", b}, {"poly", c}, {"xplan_fl", d}, {"row_score", x}, {"risk", y}, {"total", z}};
    } else if (form == "rollout_risk") {
      cilqr::plan_rollout_risk(p, B, N, M, S, delta_sets, a, b, c, d, e, o, span, base_cost, x, it, z);
      at = {{"X", a}, {"U", b}, {"k", c}, {"K", d}, {"delta", e}, {"base", base_cost}, {"risk", x}, {"step_hits", it}, {"total", z}};
    } else if (form == "declared_out_of_order") {  // a mistake a plan_* function could make: an input after an output
      p.out(x, 4);
      p.in(a, 4);
    } else if (form == "too_many_arrays") {  // B arrays of one double
      for (long j = 0; j < B; ++j) { const double* q = host_d; p.in(q, 1); }
    } else {
      fprintf(stderr, "host_plan_dump: unknown form '%s'\n", form.c_str());
      return 2;
    }
    at.push_back({"obs_pose", o.pose});
    at.push_back({"obs_dim", o.dim});
    at.push_back({"obs_weight", o.weight});
    printf("{\"ok\": %d, \"in_end\": %zu, \"out_begin\": %zu, \"end\": %zu, \"cap\": %zu, \"entries\": [", (int)p.ok, p.in_end, p.out_begin, p.end, cap);
    for (int j = 0; j < p.n; ++j)
      printf("%s[%zu, %zu, %d, %d]", j ? ", " : "", p.e[j].off, p.e[j].bytes, p.e[j].src != nullptr, p.e[j].dst != nullptr);
    printf("], \"at\": {");
    for (size_t j = 0; j < at.size(); ++j)
      printf("%s\"%s\": %ld", j ? ", " : "", at[j].first, at[j].second ? (long)((const char*)at[j].second - base) : -1L);
    printf("}}\n");
  }
  return 0;
}
