// wave_plan_dump.cpp — prints the launch plan of the one-wavefront-per-solve family (csrc/cilqr_wave_plan.h) for every shape on the
// command line, one JSON line each, for a device of 1024 SIMDs and 200 path samples.  No GPU, no HIP: tests/test_wave_plan.py.
// A shape is "name=value,…" over B N M n_samples path_samples flags map shared and the knobs of SolveKnobs.
// Batch mode for enumerations: `wave_plan_dump --stdin` reads one shape per line and prints one line of integers each,
//   kernel W long_form tab lds_fast lds_general too_large solve_wavefronts      (kernel: 0 ONE, 1 PAIR, 2 SHARE, 3 SPLIT).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cilqr_wave_plan.h"

static int dump(char* shape, bool compact) {
  cilqr::SolveKnobs k = {};
  k.simds = 1024; k.share_max = -1;
  cilqr::WaveShape s = {};
  s.path_samples = 200;
  int flags = 0, map = 0, shared = 0;
  const struct { const char* name; int* v; } fields[] = {
      {"B", &s.B}, {"N", &s.N}, {"M", &s.M}, {"n_samples", &s.n_samples}, {"path_samples", &s.path_samples}, {"flags", &flags}, {"map", &map},
      {"shared", &shared}, {"simds", &k.simds}, {"force_g", &k.force_g}, {"hint_off", &k.hint_off}, {"pair_on", &k.pair_on},
      {"steal_off", &k.steal_off}, {"split_off", &k.split_off}, {"split_w", &k.split_w}, {"share_off", &k.share_off},
      {"share_w", &k.share_w}, {"share_max", &k.share_max}, {"tab_budget_kb", &k.tab_budget_kb}};
  for (char* tok = strtok(shape, ","); tok; tok = strtok(nullptr, ",")) {
    char* eq = strchr(tok, '=');
    bool known = false;
    for (const auto& f : fields)
      if (eq && strlen(f.name) == (size_t)(eq - tok) && strncmp(f.name, tok, eq - tok) == 0) { *f.v = atoi(eq + 1); known = true; }
    if (!known) { fprintf(stderr, "wave_plan_dump: bad field '%s'\n", tok); return 2; }
  }
  s.flags = (uint32_t)flags; s.has_map = map != 0; s.obs_shared = shared != 0;
  const cilqr::WavePlan p = cilqr::plan_wave(k, s);
  const int w = cilqr::query_wavefronts(k, s.B, s.N, s.M, s.path_samples, s.has_map);
  if (compact) {
    printf("%d %d %d %d %zu %zu %d %d\n", (int)p.kernel, p.W, (int)p.long_form, p.tab, p.lds_fast, p.lds_general, (int)p.too_large, w);
    return 0;
  }
  static const char* const names[] = {"ONE", "PAIR", "SHARE", "SPLIT"};
  printf("{\"family\": %d, \"kernel\": \"%s\", \"W\": %d, \"long_form\": %d, \"tab\": %d, \"shared_table\": %d, \"lds_fast\": %zu, \"lds_general\": %zu, "
         "\"hinted\": %d, \"too_large\": %d, \"solve_wavefronts\": %d, \"solve_sampled_wavefronts\": %d}\n",
         cilqr::plan_group_lanes(k, s.B, s.N, s.M), names[p.kernel], p.W, (int)p.long_form, p.tab, (int)p.shared_table, p.lds_fast, p.lds_general,
         (int)p.hinted, (int)p.too_large, w, cilqr::split_shape_wavefronts(k, s.B, s.N, s.M));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "--stdin") == 0) {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
      line[strcspn(line, "\r\n")] = 0;
      if (const int rc = line[0] ? dump(line, true) : 0) return rc;
    }
    return 0;
  }
  for (int i = 1; i < argc; ++i)
    if (const int rc = dump(argv[i], false)) return rc;
  return 0;
}
