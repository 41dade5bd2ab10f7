// host_plan_sampled_dump.cpp — host_plan_dump.cpp for the two host forms that take sampled obstacles in compact form beyond the solve
// and the score: where the arrays of cilqr_gains_batch_sampled and cilqr_rollout_risk_sampled lie in the device arena
// (csrc/cilqr_host_plan.h), one JSON line per shape on the command line.  No GPU, no HIP: tests/test_risk_sampled.py.
// A shape is "form=NAME,name=value,…" over B N n_obs n_samples S delta_sets and the switch opt (optional outputs and `base` given);
// NAME is gains_batch_sampled or rollout_risk_sampled.  The handle is the smallest that takes the call: max_batch = max(B, 1),
// max_horizon = N, max_obstacles = n_obs*n_samples; "cap" is its arena.  Each entry prints as [offset, bytes, travels in, travels
// back]; "at" gives the offset each pointer was swapped for (-1: null).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "cilqr_host_plan.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    long B = 0, N = 1, n_obs = 1, n_samples = 2, S = 1, delta_sets = 1, opt = 0;
    std::string form;
    const struct { const char* name; long* v; } fields[] = {{"B", &B}, {"N", &N}, {"n_obs", &n_obs}, {"n_samples", &n_samples}, {"S", &S},
                                                            {"delta_sets", &delta_sets}, {"opt", &opt}};
    for (char* tok = strtok(argv[i], ","); tok; tok = strtok(nullptr, ",")) {
      char* eq = strchr(tok, '=');
      bool known = eq && strncmp(tok, "form=", 5) == 0;
      if (known) form = eq + 1;
      for (const auto& f : fields)
        if (eq && strlen(f.name) == (size_t)(eq - tok) && strncmp(f.name, tok, eq - tok) == 0) { *f.v = atol(eq + 1); known = true; }
      if (!known) { fprintf(stderr, "host_plan_sampled_dump: bad field '%s'\n", tok); return 2; }
    }
    const size_t cap = cilqr::host_arena_bytes(B > 0 ? B : 1, N, n_obs * n_samples);
    std::vector<char> arena(cap + 16);
    char* base = arena.data();
    // host pointers to declare with: never read, told apart from the arena by their addresses
    static double host_d[4];
    static int32_t host_i[4];
    const double *a = host_d, *b = host_d, *c = host_d, *d = host_d, *e = host_d, *samp = host_d, *base_cost = opt ? host_d : nullptr;
    double *x = host_d, *y = host_d, *z = opt ? host_d : nullptr;
    int32_t* it = opt ? host_i : nullptr;
    cilqr_obstacles o = {host_d, host_d, host_d, 0, 0, 0, 0};  // (a weight pointer: the plans must drop it)
    cilqr::HostPlan p(base);
    std::vector<std::pair<const char*, const void*>> at;
    if (form == "gains_batch_sampled") {
      cilqr::plan_gains_sampled(p, B, N, n_obs, n_samples, a, b, c, d, o, samp, x, y, it);
      at = {{"X", a}, {"U", b}, {"poly", c}, {"xplan_fl", d}, {"samp_off", samp}, {"k_out", x}, {"K_out", y}, {"ok_out", it}};
    } else if (form == "rollout_risk_sampled") {
      cilqr::plan_rollout_risk_sampled(p, B, N, n_obs, n_samples, S, delta_sets, a, b, c, d, e, o, samp, base_cost, x, it, z);
      at = {{"X", a}, {"U", b}, {"k", c}, {"K", d}, {"delta", e}, {"samp_off", samp}, {"base", base_cost}, {"risk", x}, {"step_hits", it}, {"total", z}};
    } else {
      fprintf(stderr, "host_plan_sampled_dump: unknown form '%s'\n", form.c_str());
      return 2;
    }
    at.push_back({"nom_pose", o.pose});
    at.push_back({"nom_dim", o.dim});
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
