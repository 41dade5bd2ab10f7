// candidates_risk_fused.cpp — iLQR::run_candidates with the fused pose-noise check (set_pose_noise_check_fused): the scene of
// candidates_risk.cpp, one static obstacle 1 m beside a straight path and candidates spread laterally across it, with 70 start
// offsets of the size of the node's pose noise.
//   1. with the check set, run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_solve_batch_obstacles,
//      cilqr_gains_batch(lamb 1), cilqr_score_batch (nominal totals), cilqr_rollout_risk(k_scale 0, max_risk, base = those totals),
//      strict-< first minimum of `total` — with X_result / U_result / last_cost of that candidate, and last_risk, last_step_hits and
//      last_scores equal to that sequence's, bit for bit;
//   2. the stored-rows sequence (cilqr_rollout_batch, cilqr_score_rollouts) on the same solves gives the same shares, worst rows and
//      worst c (bit for bit), and its rejections are the fused check's;
//   3. with every candidate rejected (max_risk = -1) the call returns -1 and X_result / U_result / last_cost are untouched;
//   4. set_pose_noise_check afterwards applies the stored-rows check again (last_step_hits empty, CILQR_RISK_FIELDS per candidate);
//      an empty offset set switches the check off.
// With a file name as its argument it writes what a checker needs to derive the pick on its own: the sizes, max_risk, the pick, then
// poly, xplan_fl, X, U, the nominal totals, the offsets, last_risk and last_step_hits, as text, one value per line.
// Prints "fused risk pick ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main(int argc, char** argv) {
  const int N = 30, M = 1, B = 16, S = 70;
  const double max_risk = 0.1;
  const int RR = CILQR_ROLLOUT_RISK_FIELDS;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, -3.0, 0.5);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 12.0, -1.0)};
  const std::vector<double> offsets = make_offsets(S);

  // by hand: the host-buffer forms on a handle whose max_batch holds the B*S rows of the stored-rows sequence
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B * S, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B), ok(B);
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};  // one set for the batch, constant over the horizon
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), Xr((size_t)B * S * 4 * (N + 1)), Ur((size_t)B * S * 2 * N);
  std::vector<double> score((size_t)B * CILQR_SCORE_FIELDS), base(B), risk((size_t)B * RR), total(B), total_none(B);
  std::vector<int32_t> hits((size_t)B * N), hits_none((size_t)B * N);
  std::vector<double> rows((size_t)B * S * CILQR_SCORE_FIELDS), risk3((size_t)B * CILQR_RISK_FIELDS), total3(B);
  const bool done =
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_obstacles(h, B, N, M, egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(),
                                  status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, score.data(), base.data()) == CILQR_OK &&
      cilqr_rollout_risk(h, B, N, M, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, &obs, -1.0, base.data(), risk.data(),
                         hits_none.data(), total_none.data()) == CILQR_OK &&
      cilqr_rollout_risk(h, B, N, M, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, &obs, max_risk, base.data(),
                         risk.data(), hits.data(), total.data()) == CILQR_OK &&
      cilqr_rollout_batch(h, B, N, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, Xr.data(), Ur.data()) == CILQR_OK &&
      cilqr_score_rollouts(h, B, N, M, S, Xr.data(), Ur.data(), poly.data(), fl.data(), &obs, max_risk, rows.data(), risk3.data(),
                           total3.data()) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  cilqr_destroy(h);
  const int want = first_minimum(total);
  int rejected = 0;
  for (int b = 0; b < B; ++b) {
    rejected += total[b] != total[b];
    const double* r = &risk[(size_t)RR * b];
    printf("candidate %2d: nominal total %.6f risk %.4f worst c %+.4f (row %g, entry %g) first step %g step share %.4f\n", b, base[b],
           r[CILQR_RR_COLLISION], r[CILQR_RR_WORST_C], r[CILQR_RR_WORST_ROW], r[CILQR_RR_WORST_ENTRY], r[CILQR_RR_FIRST_STEP],
           r[CILQR_RR_STEP_SHARE]);
  }
  printf("pick by hand: nominal total among risk <= %g: %d; %d of %d candidates rejected\n", max_risk, want, rejected, B);
  if (rejected == 0 || rejected == B || want < 0 || first_minimum(total_none) != -1) {
    printf("the scene does not separate the candidates by risk\n");
    return 1;
  }
  if (memcmp(hits.data(), hits_none.data(), hits.size() * sizeof(int32_t)) != 0) { printf("step_hits depend on max_risk\n"); return 1; }
  // 2. the stored-rows sequence on the same solves
  for (int b = 0; b < B; ++b) {
    const double *r = &risk[(size_t)RR * b], *r3 = &risk3[(size_t)CILQR_RISK_FIELDS * b];
    const int row = (int)r3[CILQR_RISK_WORST_ROW];
    if (!same(&r[CILQR_RR_COLLISION], &r3[CILQR_RISK_COLLISION], 1) || !same(&r[CILQR_RR_WORST_C], &r3[CILQR_RISK_WORST_C], 1) ||
        r[CILQR_RR_WORST_ROW] != r3[CILQR_RISK_WORST_ROW] ||
        r[CILQR_RR_WORST_ENTRY] != rows[((size_t)b * S + row) * CILQR_SCORE_FIELDS + CILQR_SCORE_MAX_C_ENTRY] ||
        (total[b] != total[b]) != (total3[b] != total3[b])) {
      printf("candidate %d: the fused risk differs from cilqr_score_rollouts\n", b);
      return 1;
    }
  }

  iLQR planner(params, 0, M, B);
  planner.set_global_plan(path);
  planner.set_Obstacle(obstacles);
  // 1. the check set
  planner.set_pose_noise_check_fused(offsets, max_risk);
  const int best = planner.run_candidates(egos);
  if (best != want) { printf("the check picked %d, the sequence by hand %d\n", best, want); return 1; }
  if (planner.last_risk.size() != risk.size() || !same(planner.last_risk.data(), risk.data(), risk.size())) {
    printf("last_risk differs from cilqr_rollout_risk on the same solves\n");
    return 1;
  }
  if (planner.last_step_hits.size() != hits.size() || memcmp(planner.last_step_hits.data(), hits.data(), hits.size() * sizeof(int32_t)) != 0) {
    printf("last_step_hits differs from cilqr_rollout_risk on the same solves\n");
    return 1;
  }
  if (planner.last_scores.size() != score.size() || !same(planner.last_scores.data(), score.data(), score.size())) {
    printf("last_scores differs from cilqr_score_batch on the same solves\n");
    return 1;
  }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best]) {
    printf("the pick's X / U / J differ from the hand-written solve\n");
    return 1;
  }
  if (argc > 1) {
    FILE* f = fopen(argv[1], "w");
    if (!f) { printf("cannot write %s\n", argv[1]); return 1; }
    fprintf(f, "%d\n%d\n%d\n%d\n%.17g\n%d\n", B, N, M, S, max_risk, best);
    put(f, poly); put(f, fl); put(f, X); put(f, U); put(f, base); put(f, offsets); put(f, planner.last_risk);
    for (int32_t v : planner.last_step_hits) fprintf(f, "%d\n", (int)v);
    fclose(f);
  }
  // 3. every candidate rejected
  const Matrix X_before = planner.X_result, U_before = planner.U_result, ref_before = planner.ref_traj_result;
  const double cost_before = planner.last_cost;
  const int it_before = planner.last_iterations, exit_before = planner.last_exit;
  planner.set_pose_noise_check_fused(offsets, -1.0);
  const int none = planner.run_candidates(egos);
  if (none != -1) { printf("every candidate rejected, yet the pick is %d\n", none); return 1; }
  if (!same(planner.U_result.a.data(), U_before.a.data(), U_before.a.size()) ||
      !same(planner.X_result.a.data(), X_before.a.data(), X_before.a.size()) ||
      !same(planner.ref_traj_result.a.data(), ref_before.a.data(), ref_before.a.size()) || !same(&planner.last_cost, &cost_before, 1) ||
      planner.last_iterations != it_before || planner.last_exit != exit_before || planner.last_risk.size() != risk.size() ||
      planner.last_step_hits.size() != hits.size()) {
    printf("all rejected: results were touched\n");
    return 1;
  }
  // 4. the stored-rows check set afterwards applies; then switched off: the default pick by J.  (The warm start is the first pick's U
  // now, so only the modes are checked.)
  planner.set_pose_noise_check(offsets, 1.0);
  const int stored = planner.run_candidates(egos);
  if (stored < 0 || planner.last_risk.size() != (size_t)B * CILQR_RISK_FIELDS || !planner.last_step_hits.empty() || !planner.last_scores.empty()) {
    printf("stored-rows check after the fused one: pick %d, %zu risk values\n", stored, planner.last_risk.size());
    return 1;
  }
  planner.set_pose_noise_check_fused({}, 1.0);
  const int plain = planner.run_candidates(egos);
  if (plain < 0 || !planner.last_risk.empty() || !planner.last_step_hits.empty()) { printf("check off: pick %d, last_risk not empty\n", plain); return 1; }
  printf("fused risk pick ok\n");
  return 0;
}
