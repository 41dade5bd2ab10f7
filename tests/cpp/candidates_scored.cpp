// candidates_scored.cpp — iLQR::run_candidates with the opt-in pick by total cost (set_candidate_pick): one static obstacle 1 m beside
// a straight path, candidates spread laterally from 3 m on its side to 4.5 m on the other.  The candidate that tracks best drives
// through the inflated obstacle; its neighbour passes clear of it.
//   1. the default pick (MinTrackingCost) is what run_candidates did before the option existed: the strict-< first minimum of J over
//      a hand-written cilqr_solve_batch_obstacles of the same candidates, X / U / J bit for bit, and last_scores stays empty;
//   2. MinTotalCost with max_collision = 0 returns a candidate whose last_scores row has COLLISION 0, and that candidate is the
//      host-side minimum over the `total` column a hand-written cilqr_score_batch gives for the same solves; last_scores equals
//      that call's rows bit for bit;
//   3. with every candidate rejected (max_collision = -1) the call returns -1 and X_result / U_result / last_cost are untouched.
// Prints "scored pick ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 30, M = 1, B = 16;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, -3.0, 0.5);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 12.0, -1.0)};

  // by hand: the same pre-step and solve, then the scores
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B);
  if (cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) != CILQR_OK) {
    printf("cilqr_local_plan_batch: %s\n", cilqr_last_error());
    return 1;
  }
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};  // one set for the batch, constant over the horizon
  if (cilqr_solve_batch_obstacles(h, B, N, M, egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(),
                                  status.data(), CILQR_FLAG_NONE) != CILQR_OK) {
    printf("cilqr_solve_batch_obstacles: %s\n", cilqr_last_error());
    return 1;
  }
  std::vector<double> score((size_t)B * CILQR_SCORE_FIELDS), total(B), total_all(B);
  if (cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 0.0, score.data(), total.data()) != CILQR_OK ||
      cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, score.data(), total_all.data()) != CILQR_OK) {
    printf("cilqr_score_batch: %s\n", cilqr_last_error());
    return 1;
  }
  cilqr_destroy(h);
  const int want_j = first_minimum(J), want_safe = first_minimum(total), want_total = first_minimum(total_all);
  int colliding = 0;
  for (int b = 0; b < B; ++b) {
    colliding += score[(size_t)b * CILQR_SCORE_FIELDS + CILQR_SCORE_COLLISION] > 0.0;
    printf("candidate %2d: J %.6f total %.6f max c %+.4f collision %g\n", b, J[b], total_all[b],
           score[(size_t)b * CILQR_SCORE_FIELDS + CILQR_SCORE_MAX_C], score[(size_t)b * CILQR_SCORE_FIELDS + CILQR_SCORE_COLLISION]);
  }
  printf("picks by hand: J %d, total %d, total among the safe %d; %d of %d candidates in contact\n", want_j, want_total, want_safe, colliding, B);
  if (colliding == 0 || colliding == B || want_safe < 0 || want_safe == want_j) {
    printf("the scene does not separate the safe pick from the pick by J\n");
    return 1;
  }

  // 1. default pick
  {
    iLQR planner(params, 0, M, B);
    planner.set_global_plan(path);
    planner.set_Obstacle(obstacles);
    const int best = planner.run_candidates(egos);
    if (best != want_j || !planner.last_scores.empty()) { printf("default pick %d, by hand %d\n", best, want_j); return 1; }
    if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
        !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1)) {
      printf("default pick: X / U / J differ from the hand-written solve\n");
      return 1;
    }
  }
  // 2. total cost among the candidates without contact; 3. every candidate rejected
  {
    iLQR planner(params, 0, M, B);
    planner.set_global_plan(path);
    planner.set_Obstacle(obstacles);
    planner.set_candidate_pick(CandidatePick::MinTotalCost);  // max_collision = 0
    const int best = planner.run_candidates(egos);
    if (best != want_safe) { printf("MinTotalCost picked %d, the host-side minimum over total is %d\n", best, want_safe); return 1; }
    if (planner.last_scores.size() != score.size() || !same(planner.last_scores.data(), score.data(), score.size())) {
      printf("last_scores differ from cilqr_score_batch on the same solves\n");
      return 1;
    }
    if (planner.last_scores[(size_t)best * CILQR_SCORE_FIELDS + CILQR_SCORE_COLLISION] != 0.0) { printf("the pick is in contact\n"); return 1; }
    if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
        !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N)) {
      printf("MinTotalCost: X / U of the pick differ from the hand-written solve\n");
      return 1;
    }
    const Matrix X_before = planner.X_result, U_before = planner.U_result;
    const double cost_before = planner.last_cost;
    planner.set_candidate_pick(CandidatePick::MinTotalCost, -1.0);
    const int none = planner.run_candidates(egos);
    if (none != -1) { printf("every candidate rejected, yet the pick is %d\n", none); return 1; }
    if (!same(planner.U_result.a.data(), U_before.a.data(), U_before.a.size()) ||
        !same(planner.X_result.a.data(), X_before.a.data(), X_before.a.size()) || !same(&planner.last_cost, &cost_before, 1) ||
        planner.last_scores.size() != score.size()) {
      printf("all rejected: results were touched\n");
      return 1;
    }
  }
  printf("scored pick ok\n");
  return 0;
}
