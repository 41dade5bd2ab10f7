// candidates_risk_sampled.cpp — iLQR with sampled obstacles (set_obstacle_samples): four candidates beside a straight path, one
// nominal obstacle 2.5 m to its right with 8 pose samples (sigma 0.45 m, 0.05 rad) shared by the candidates, 70 ego start offsets of
// the size of the node's pose noise.
//   1. under set_pose_noise_check_fused, run_candidates returns the index the C-ABI sequence called by hand gives —
//      cilqr_solve_batch_sampled, cilqr_gains_batch_sampled(lamb 1), cilqr_score_batch_sampled (nominal totals, max_collision 1),
//      cilqr_rollout_risk_sampled(k_scale 0, max_risk, base = those totals), strict-< first minimum of `total` — with X_result /
//      U_result / last_cost of that candidate, and last_risk (CILQR_RRS_FIELDS per candidate), last_step_hits and last_scores equal to
//      that sequence's, bit for bit; the bound rejects some candidates and not all;
//   2. run_step and run_candidates (MinTotalCost, no pose-noise check) with samples set solve and score in the sampled form;
//   3. with samples set, set_pose_noise_check throws std::logic_error naming set_pose_noise_check_fused, also when the samples are
//      set after it and run_candidates is called;
//   4. with the samples cleared, a planner gives what a planner that never had samples gives, bit for bit (fused check, stored-rows
//      check, no check).
// With a file name as its argument it writes what a checker needs to repeat the calls: the sizes, max_risk, the pick, then the ego
// states, the warm start, poly, xplan_fl, X, U, the nominal obstacle tables, the sample offsets, the ego offsets, last_risk,
// last_step_hits and last_scores, as text, one value per line.
// Prints "sampled risk pick ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
bool results_equal(const iLQR& a, const iLQR& b) {
  return same(a.X_result.a, b.X_result.a) && same(a.U_result.a, b.U_result.a) && same(&a.last_cost, &b.last_cost, 1) &&
         a.last_iterations == b.last_iterations && a.last_exit == b.last_exit && same(a.last_risk, b.last_risk) &&
         same(a.last_scores, b.last_scores) && a.last_step_hits == b.last_step_hits;
}
}  // namespace

int main(int argc, char** argv) {
  const int N = 30, n_obs = 1, ns = 8, M = n_obs * ns, B = 4, S = 70;
  const double max_risk = 0.1;
  const int F = CILQR_RRS_FIELDS;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, 0.0, 0.6);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 12.0, -2.5)};
  Draws draws;
  const std::vector<double> offsets = make_offsets(S, draws), samples = make_pose_samples(n_obs * ns, draws);
  const double weight = params.w_obstacle / ns;

  // by hand: the host-buffer forms, the obstacle set repeated for every candidate
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), X((size_t)B * 4 * (N + 1)), J(B);
  const std::vector<double> U0 = default_controls(B, N);
  std::vector<int32_t> iters(B), status(B), ok(B);
  std::vector<double> U = U0;
  std::vector<double> nom_pose((size_t)B * n_obs * 4 * N), nom_dim((size_t)B * n_obs * 2 * N), off((size_t)B * samples.size());
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < N; ++t) {
      for (int r = 0; r < 4; ++r) nom_pose[((size_t)b * N + t) * 4 + r] = obstacles[0].relative_pos_array(r, t);
      for (int r = 0; r < 2; ++r) nom_dim[((size_t)b * N + t) * 2 + r] = obstacles[0].dimension(r, t);
    }
    memcpy(&off[(size_t)b * samples.size()], samples.data(), samples.size() * sizeof(double));
  }
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), score((size_t)B * CILQR_SCORE_FIELDS), base(B), risk((size_t)B * F), total(B);
  std::vector<double> score0((size_t)B * CILQR_SCORE_FIELDS), total0(B), X1(4 * (size_t)(N + 1)), U1(U0.begin(), U0.begin() + 2 * N);
  std::vector<int32_t> hits((size_t)B * N);
  double J1 = 0.0;
  int32_t it1 = 0, st1 = 0;
  const bool done =
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_sampled(h, B, N, n_obs, ns, egos.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, X.data(), J.data(), iters.data(), status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch_sampled(h, B, N, n_obs, ns, X.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_score_batch_sampled(h, B, N, n_obs, ns, X.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, 1.0, score.data(), base.data()) == CILQR_OK &&
      cilqr_rollout_risk_sampled(h, B, N, n_obs, ns, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, nom_pose.data(),
                                 nom_dim.data(), off.data(), max_risk, base.data(), risk.data(), hits.data(), total.data()) == CILQR_OK &&
      cilqr_score_batch_sampled(h, B, N, n_obs, ns, X.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, 0.2, score0.data(), total0.data()) == CILQR_OK &&
      // (candidate 0 alone, as run_step solves it)
      cilqr_solve_batch_sampled(h, 1, N, n_obs, ns, egos.data(), U1.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, X1.data(), &J1, &it1, &st1, CILQR_FLAG_NONE) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  cilqr_destroy(h);
  const int want = first_minimum(total);
  int rejected = 0;
  for (int b = 0; b < B; ++b) {
    rejected += total[b] != total[b];
    const double* r = &risk[(size_t)F * b];
    printf("candidate %d: nominal total %.6f collision %.4f worst c %+.4f (row %g, entry %g) first step %g step share %.4f any %.4f pair %.4f\n", b,
           base[b], r[CILQR_RRS_COLLISION], r[CILQR_RRS_WORST_C], r[CILQR_RRS_WORST_ROW], r[CILQR_RRS_WORST_ENTRY], r[CILQR_RRS_FIRST_STEP],
           r[CILQR_RRS_STEP_SHARE], r[CILQR_RRS_ANY_SHARE], r[CILQR_RRS_PAIR_SHARE]);
  }
  printf("pick by hand: nominal total among collision <= %g: %d; %d of %d candidates rejected\n", max_risk, want, rejected, B);
  if (rejected == 0 || rejected == B || want < 0) { printf("the scene does not separate the candidates by risk\n"); return 1; }

  // 1. the fused check with samples set
  iLQR planner(params, 0, M, B);
  planner.set_global_plan(path);
  planner.set_Obstacle(obstacles);
  planner.set_obstacle_samples(samples, ns);
  planner.set_pose_noise_check_fused(offsets, max_risk);
  const int best = planner.run_candidates(egos);
  if (best != want) { printf("the check picked %d, the sequence by hand %d\n", best, want); return 1; }
  if (!same(planner.last_risk, risk)) { printf("last_risk differs from cilqr_rollout_risk_sampled on the same solves\n"); return 1; }
  if (planner.last_step_hits != hits) { printf("last_step_hits differs from cilqr_rollout_risk_sampled on the same solves\n"); return 1; }
  if (!same(planner.last_scores, score)) { printf("last_scores differs from cilqr_score_batch_sampled on the same solves\n"); return 1; }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best]) {
    printf("the pick's X / U / J differ from the hand-written solve\n");
    return 1;
  }
  if (argc > 1) {
    FILE* f = fopen(argv[1], "w");
    if (!f) { printf("cannot write %s\n", argv[1]); return 1; }
    fprintf(f, "%d\n%d\n%d\n%d\n%d\n%.17g\n%d\n", B, N, n_obs, ns, S, max_risk, best);
    put(f, egos); put(f, U0); put(f, poly); put(f, fl); put(f, X); put(f, U);
    put(f, std::vector<double>(nom_pose.begin(), nom_pose.begin() + (size_t)n_obs * 4 * N));
    put(f, std::vector<double>(nom_dim.begin(), nom_dim.begin() + (size_t)n_obs * 2 * N));
    put(f, samples); put(f, offsets); put(f, planner.last_risk);
    for (int32_t v : planner.last_step_hits) fprintf(f, "%d\n", (int)v);
    put(f, planner.last_scores);
    fclose(f);
  }

  // 2. run_step and the MinTotalCost pick in the sampled form
  {
    iLQR q(params, 0, M, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    q.set_obstacle_samples(samples, ns);
    q.run_step(egos.data());
    if (!same(q.X_result.a.data(), X1.data(), X1.size()) || !same(q.U_result.a.data(), U1.data(), U1.size()) || !same(&q.last_cost, &J1, 1) ||
        q.last_iterations != it1 || q.last_exit != st1) {
      printf("run_step with samples differs from cilqr_solve_batch_sampled\n");
      return 1;
    }
    iLQR c(params, 0, M, B);
    c.set_global_plan(path);
    c.set_Obstacle(obstacles);
    c.set_obstacle_samples(samples, ns);
    c.set_candidate_pick(CandidatePick::MinTotalCost, 0.2);
    const int pick = c.run_candidates(egos);
    if (pick != first_minimum(total0) || !same(c.last_scores, score0) || !c.last_risk.empty()) {
      printf("MinTotalCost with samples: pick %d, by hand %d\n", pick, first_minimum(total0));
      return 1;
    }
  }

  // 3. the stored-rows check has no sampled form
  {
    bool threw = false;
    try {
      planner.set_pose_noise_check(offsets, 1.0);
    } catch (const std::logic_error& e) {
      threw = strstr(e.what(), "set_pose_noise_check_fused") != nullptr;
    }
    if (!threw) { printf("set_pose_noise_check with samples set did not throw a logic_error naming the fused setter\n"); return 1; }
    iLQR q(params, 0, M, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    q.set_pose_noise_check(offsets, 1.0);
    q.set_obstacle_samples(samples, ns);
    threw = false;
    try {
      q.run_candidates(egos);
    } catch (const std::logic_error& e) {
      threw = strstr(e.what(), "set_pose_noise_check_fused") != nullptr;
    }
    if (!threw) { printf("run_candidates under the stored-rows check with samples set did not throw\n"); return 1; }
  }

  // 4. samples cleared: a planner that had samples against one that never had any (fresh planners: the same warm start)
  for (int mode = 0; mode < 3; ++mode) {
    iLQR a(params, 0, M, B), b(params, 0, M, B);
    for (iLQR* q : {&a, &b}) {
      q->set_global_plan(path);
      q->set_Obstacle(obstacles);
    }
    a.set_obstacle_samples(samples, ns);
    if (mode == 0) a.set_pose_noise_check_fused(offsets, 1.0);
    a.set_obstacle_samples({}, 0);
    for (iLQR* q : {&a, &b}) {
      if (mode == 0) q->set_pose_noise_check_fused(offsets, 1.0);
      if (mode == 1) q->set_pose_noise_check(offsets, 1.0);
      if (mode == 2) q->set_candidate_pick(CandidatePick::MinTotalCost, 1.0);
    }
    const int pa = a.run_candidates(egos), pb = b.run_candidates(egos);
    const size_t fields = mode == 0 ? CILQR_ROLLOUT_RISK_FIELDS : mode == 1 ? CILQR_RISK_FIELDS : 0;
    if (pa != pb || pa < 0 || !results_equal(a, b) || a.last_risk.size() != (size_t)B * fields) {
      printf("samples cleared (mode %d): pick %d against %d of a planner that never had samples\n", mode, pa, pb);
      return 1;
    }
    a.run_step(egos.data());
    b.run_step(egos.data());
    if (!same(a.X_result.a, b.X_result.a) || !same(a.U_result.a, b.U_result.a)) { printf("samples cleared (mode %d): run_step differs\n", mode); return 1; }
  }
  printf("sampled risk pick ok\n");
  return 0;
}
