// candidate_layout_stop_dump.cpp — candidate_layout_map_clearance_dump.cpp with the stop fallback's flag, predicate and arrays, for
// tests/test_stop_plans.py: host/candidate_layout.h on the host, no library, no GPU.  `stop_fallback` is the LAST flag bit and
// `stop_fallback_check` the last predicate bit, and the stage's arrays lie behind every earlier array, so a record of the earlier
// dumps means the same here with the flag off.
//   candidate_layout_stop_dump names    the flags, the predicates, the arrays and the stop arrays, one line each, in the order of the records
//   candidate_layout_stop_dump          reads records of 9 uint64 from stdin — the flags as bits, then B, N, M, S, n_obs, n_samples, Q, D — and
//                                       writes for each the predicates as bits, every array's offset, every stop array's offset and `end`
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "candidate_layout.h"

using cilqr_host::CandidateLayout;
using cilqr_host::CandidateModes;
using cilqr_host::CandidateSizes;

#define FLAGS(F)                                                                                                                 \
  F(noise) F(fused) F(cov) F(scov) F(sampled) F(cov_judge) F(cmap) F(map) F(tighten) F(map_tighten) F(track_map) F(min_total) \
  F(map_set) F(obstacles) F(tracks) F(footprint) F(map_clearance) F(stop_fallback)
#define PREDICATES(F)                                                                                                              \
  F(in_block) F(plain) F(sampled_solve) F(obstacle_rounds) F(map_rounds) F(track_rounds) F(rounds) F(scored) F(score_before_gains) \
  F(gains) F(stored_rows_risk) F(fused_risk) F(fused_sampled_risk) F(chance) F(chance_sampled) F(map_covariance) F(map_rollout_risk) F(footprint_check) \
  F(map_clearance_check) F(stop_fallback_check)

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "names")) {
#define F(name) printf(" " #name);
    printf("flags:"); FLAGS(F) printf("\npredicates:"); PREDICATES(F) printf("\narrays:"); CILQR_CANDIDATE_ARRAYS(F)
    printf("\nstop:"); CILQR_CANDIDATE_STOP_ARRAYS(F) printf(" end\n");
#undef F
    return 0;
  }
  uint64_t in[9];
  while (fread(in, sizeof(uint64_t), 9, stdin) == 9) {
    CandidateModes m;
    int bit = 0;
#define F(name) m.name = (in[0] >> bit++) & 1;
    FLAGS(F)
#undef F
    CandidateSizes z;
    z.B = in[1]; z.N = in[2]; z.M = in[3]; z.S = in[4]; z.n_obs = in[5]; z.n_samples = in[6]; z.Q = in[7]; z.D = in[8];
    const CandidateLayout L = cilqr_host::candidate_layout(m, z);
    uint64_t out[96], n = 1;
    out[0] = 0;
    bit = 0;
#define F(name) out[0] |= (uint64_t)m.name() << bit++;
    PREDICATES(F)
#undef F
#define F(name) out[n++] = L.name;
    CILQR_CANDIDATE_ARRAYS(F)
    CILQR_CANDIDATE_STOP_ARRAYS(F)
#undef F
    out[n++] = L.end;
    fwrite(out, sizeof(uint64_t), n, stdout);
  }
  return 0;
}
