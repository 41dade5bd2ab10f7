// candidates_footprint.cpp — iLQR::run_candidates with the footprint check (set_footprint_check) as the last gate: six candidates
// x0 = (0, -0.3 b, 5, 0) beside a straight path, one 0.5 x 0.5 m post standing at (8, 1.2), horizon 40.  The surrogate of the score
// call (an ego circle's centre inside the inflated ellipse) calls all six plans collisions; the exact check finds every one of them
// more than a metre clear.  The constants below are asserted from the CPU oracle's solves in tests/test_footprint.py.
//   1. set_candidate_pick(MinTotalCost, 0.0) alone returns -1: "no plan";
//   2. with set_footprint_check(0.5, +inf) and max_collision 1.0 the pick is the cheapest plan by total, kPickLow; last_footprint
//      equals, bit for bit, the rows of a hand-written solve -> score -> cilqr_footprint_check of the same candidates, and the pick
//      is the host-side minimum over that call's total;
//   3. at min_clearance 1.11, between the clearances of candidates 2 and 3, the pick moves to the cheapest of those left, kPickBetween;
//   4. at min_clearance 2.0 every candidate is rejected: -1;
//   5. the check alone, under the default pick, ranks by J (its base where no check ran);
//   6. with set_obstacle_samples the run throws std::logic_error.
// Prints "clearances: ..." and "footprint pick ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 40, M = 1, B = 6, kPickLow = 2, kPickBetween = 3;
  const double kBetween = 1.11, inf = INFINITY;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, 0.0, -0.3);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 8.0, 1.2, 0.0, 0.5, 0.5)};

  // by hand: the same pre-step and solve, the score's total with nothing rejected, the footprint check on top of it
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B);
  const double pose1[4] = {8.0, 1.2, 0.0, 0.0}, dim1[2] = {0.5, 0.5};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};
  std::vector<double> score((size_t)B * CILQR_SCORE_FIELDS), safe(B), all(B), fp((size_t)B * CILQR_FOOTPRINT_FIELDS), clr((size_t)B * N), low(B), between(B), by_j(B);
  if (cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) != CILQR_OK ||
      cilqr_solve_batch_obstacles(h, B, N, M, egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(), status.data(),
                                  CILQR_FLAG_NONE) != CILQR_OK ||
      cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 0.0, score.data(), safe.data()) != CILQR_OK ||
      cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, score.data(), all.data()) != CILQR_OK ||
      cilqr_footprint_check(h, B, N, M, 1, X.data(), &obs, 0.0, 0.5, inf, 0u, all.data(), fp.data(), clr.data(), nullptr, low.data()) != CILQR_OK ||
      cilqr_footprint_check(h, B, N, M, 1, X.data(), &obs, 0.0, kBetween, inf, 0u, all.data(), fp.data(), clr.data(), nullptr, between.data()) != CILQR_OK ||
      cilqr_footprint_check(h, B, N, M, 1, X.data(), &obs, 0.0, 0.5, inf, 0u, J.data(), fp.data(), clr.data(), nullptr, by_j.data()) != CILQR_OK) {
    printf("by hand: %s\n", cilqr_last_error());
    return 1;
  }
  cilqr_destroy(h);
  printf("clearances:");
  for (int b = 0; b < B; ++b) printf(" %.9f", fp[(size_t)b * CILQR_FOOTPRINT_FIELDS + CILQR_FP_CLEARANCE]);
  printf("\n");
  for (int b = 0; b < B; ++b)
    printf("candidate %d: J %.4f total %.4f collision %g hit steps %g\n", b, J[b], all[b], score[(size_t)b * CILQR_SCORE_FIELDS + CILQR_SCORE_COLLISION],
           fp[(size_t)b * CILQR_FOOTPRINT_FIELDS + CILQR_FP_HIT_STEPS]);
  if (first_minimum(safe) != -1 || count_nan(low) != 0 || first_minimum(low) != kPickLow || count_nan(between) != 3 || first_minimum(between) != kPickBetween) {
    printf("by hand: the scene is not the one the constants were taken from (picks %d %d %d)\n", first_minimum(safe), first_minimum(low), first_minimum(between));
    return 1;
  }

  iLQR planner(params, 0, M, B);
  planner.set_global_plan(path);
  planner.set_Obstacle(obstacles);
  // 1. the surrogate alone: no plan
  planner.set_candidate_pick(CandidatePick::MinTotalCost, 0.0);
  if (planner.run_candidates(egos) != -1 || !planner.last_footprint.empty()) { printf("MinTotalCost, 0.0 alone: a plan was picked\n"); return 1; }
  // 2. the exact check in its place
  planner.set_candidate_pick(CandidatePick::MinTotalCost, 1.0);
  planner.set_footprint_check(0.5, inf);
  int best = planner.run_candidates(egos);
  if (best != kPickLow) { printf("min_clearance 0.5: picked %d, the cheapest clear plan is %d\n", best, kPickLow); return 1; }
  if (!same(planner.last_footprint, fp) || !same(planner.last_footprint_clearance, clr)) { printf("last_footprint differs from cilqr_footprint_check on the same solves\n"); return 1; }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1))) { printf("the pick's X differs from the hand-written solve\n"); return 1; }
  // (a run that picks installs the pick's controls as the next warm start: each case below starts from a fresh planner)
  // 3. between candidates 2 and 3
  {
    iLQR q(params, 0, M, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    q.set_candidate_pick(CandidatePick::MinTotalCost, 1.0);
    q.set_footprint_check(kBetween, inf);
    best = q.run_candidates(egos);
    if (best != kPickBetween || !same(q.last_footprint, fp)) { printf("min_clearance %.2f: picked %d, the cheapest of those left is %d\n", kBetween, best, kPickBetween); return 1; }
    // 4. nobody is two metres clear (a rejected run leaves the warm start as it was: the rows are those of the run before)
    const Matrix X_before = q.X_result;
    q.set_footprint_check(2.0, inf);
    if (q.run_candidates(egos) != -1 || q.last_footprint.size() != fp.size() || !same(q.X_result.a, X_before.a)) { printf("min_clearance 2.0: a plan was picked\n"); return 1; }
  }
  // 5. the check alone: its base is J
  {
    iLQR q(params, 0, M, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    q.set_footprint_check(0.5, inf);
    best = q.run_candidates(egos);
    if (best != first_minimum(by_j) || !q.last_scores.empty() || !same(q.last_footprint, fp)) { printf("the check alone: picked %d, by J %d\n", best, first_minimum(by_j)); return 1; }
  }
  // ... and switched off the run is what it was
  {
    iLQR q(params, 0, M, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    q.set_footprint_check(0.5, inf);
    q.set_footprint_check(0.5, inf, 0.0, false, false);
    best = q.run_candidates(egos);
    if (best != first_minimum(J) || !q.last_footprint.empty()) { printf("switched off: picked %d, by J %d\n", best, first_minimum(J)); return 1; }
  }
  // 6. no sampled form
  {
    iLQR q(params, 0, 4, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    Draws draws;
    q.set_obstacle_samples(make_pose_samples(2, draws), 2);
    q.set_footprint_check(0.5, inf);
    if (!throws_logic_error([&] { q.run_candidates(egos); }, "set_footprint_check")) { printf("with set_obstacle_samples the run did not throw\n"); return 1; }
  }
  printf("footprint pick ok\n");
  return 0;
}
