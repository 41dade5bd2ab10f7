// candidates_risk.cpp — iLQR::run_candidates with the pose-noise check (set_pose_noise_check): the scene of candidates_scored.cpp, one
// static obstacle 1 m beside a straight path and candidates spread laterally across it, with 70 start offsets of the size of the
// node's pose noise.
//   1. with the check set, run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_solve_batch_obstacles,
//      cilqr_gains_batch(lamb 1), cilqr_rollout_batch(k_scale 0), cilqr_score_rollouts(max_risk), strict-< first minimum of `total` —
//      with X_result / U_result / last_cost of that candidate and last_risk equal to that sequence's risk rows, bit for bit;
//   2. with every candidate rejected (max_risk = -1) the call returns -1 and X_result / U_result / last_cost are untouched;
//   3. an empty offset set switches the check off: the default pick again.
// Prints "risk pick ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 30, M = 1, B = 16, S = 70;
  const double max_risk = 0.1;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, -3.0, 0.5);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 12.0, -1.0)};
  const std::vector<double> offsets = make_offsets(S);

  // by hand: the host-buffer forms on a handle whose max_batch holds the B*S rows
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B * S, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B), ok(B);
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};  // one set for the batch, constant over the horizon
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), Xr((size_t)B * S * 4 * (N + 1)), Ur((size_t)B * S * 2 * N);
  std::vector<double> rows((size_t)B * S * CILQR_SCORE_FIELDS), risk((size_t)B * CILQR_RISK_FIELDS), total(B), total_none(B);
  const bool done =
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_obstacles(h, B, N, M, egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(),
                                  status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_rollout_batch(h, B, N, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, Xr.data(), Ur.data()) == CILQR_OK &&
      cilqr_score_rollouts(h, B, N, M, S, Xr.data(), Ur.data(), poly.data(), fl.data(), &obs, -1.0, rows.data(), risk.data(),
                           total_none.data()) == CILQR_OK &&
      cilqr_score_rollouts(h, B, N, M, S, Xr.data(), Ur.data(), poly.data(), fl.data(), &obs, max_risk, rows.data(), risk.data(),
                           total.data()) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  cilqr_destroy(h);
  const int want = first_minimum(total), want_j = first_minimum(J);
  int rejected = 0;
  for (int b = 0; b < B; ++b) {
    rejected += total[b] != total[b];
    printf("candidate %2d: J %.6f risk %.4f worst c %+.4f (row %g) mean total %.6f gains ok %d\n", b, J[b], risk[4 * b + CILQR_RISK_COLLISION],
           risk[4 * b + CILQR_RISK_WORST_C], risk[4 * b + CILQR_RISK_WORST_ROW], risk[4 * b + CILQR_RISK_MEAN_TOTAL], ok[b]);
  }
  printf("picks by hand: J %d, mean total among risk <= %g: %d; %d of %d candidates rejected\n", want_j, max_risk, want, rejected, B);
  if (rejected == 0 || rejected == B || want < 0 || first_minimum(total_none) != -1) {
    printf("the scene does not separate the candidates by risk\n");
    return 1;
  }

  iLQR planner(params, 0, M, B);
  planner.set_global_plan(path);
  planner.set_Obstacle(obstacles);
  // 1. the check set
  planner.set_pose_noise_check(offsets, max_risk);
  const int best = planner.run_candidates(egos);
  if (best != want) { printf("the check picked %d, the sequence by hand %d\n", best, want); return 1; }
  if (planner.last_risk.size() != risk.size() || !same(planner.last_risk.data(), risk.data(), risk.size())) {
    printf("last_risk differs from cilqr_score_rollouts on the same solves\n");
    return 1;
  }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best] || !planner.last_scores.empty()) {
    printf("the pick's X / U / J differ from the hand-written solve\n");
    return 1;
  }
  // 2. every candidate rejected
  const Matrix X_before = planner.X_result, U_before = planner.U_result, ref_before = planner.ref_traj_result;
  const double cost_before = planner.last_cost;
  const int it_before = planner.last_iterations, exit_before = planner.last_exit;
  planner.set_pose_noise_check(offsets, -1.0);
  const int none = planner.run_candidates(egos);
  if (none != -1) { printf("every candidate rejected, yet the pick is %d\n", none); return 1; }
  if (!same(planner.U_result.a.data(), U_before.a.data(), U_before.a.size()) ||
      !same(planner.X_result.a.data(), X_before.a.data(), X_before.a.size()) ||
      !same(planner.ref_traj_result.a.data(), ref_before.a.data(), ref_before.a.size()) || !same(&planner.last_cost, &cost_before, 1) ||
      planner.last_iterations != it_before || planner.last_exit != exit_before || planner.last_risk.size() != risk.size()) {
    printf("all rejected: results were touched\n");
    return 1;
  }
  // 3. switched off again: the default pick by J.  (The warm start is the first pick's U now, so only the mode is checked.)
  planner.set_pose_noise_check({}, 1.0);
  const int plain = planner.run_candidates(egos);
  if (plain < 0 || !planner.last_risk.empty()) { printf("check off: pick %d, last_risk not empty\n", plain); return 1; }
  printf("risk pick ok\n");
  return 0;
}
