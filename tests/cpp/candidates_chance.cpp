// candidates_chance.cpp — iLQR::run_candidates with the pose-covariance check (set_pose_covariance_check): the scene of
// candidates_risk_fused.cpp, one static obstacle 1 m beside a straight path and candidates spread laterally across it, with the node's
// pose noise given as a covariance, Sigma0 = diag(0.16^2, 0.16^2, 0, 0.017^2), and a small process noise.
//   1. with the check set, run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_solve_batch_obstacles,
//      (under MinTotalCost cilqr_score_batch, max_collision 1) cilqr_gains_batch(lamb 1), cilqr_chance_risk(max_risk, base = J or those
//      totals), strict-< first minimum of `total` — with X_result / U_result / last_cost of that candidate, and last_chance_risk,
//      last_step_risk and last_scores equal to that sequence's, bit for bit; under MinTrackingCost, under MinTotalCost, with
//      sum_bound, and with an uncertainty map set and set_map_risk_check composing after it (cilqr_rollout_risk_map on ONE zero
//      offset, base = the chance total);
//   2. with every candidate rejected (max_risk = -1) the call returns -1 and X_result / U_result / last_cost are untouched;
//   3. Sigma0 == nullptr switches the check off;
//   4. together with set_pose_noise_check(_fused) offsets or set_obstacle_samples, whichever comes second throws std::logic_error;
//   5. params.horizon lowered to 12 after a checked run: the next run equals the sequence by hand at that horizon, from the first 12
//      steps of the warm start the first run left (the device block is laid out anew).
// Prints "chance pick ok" and "conflicts throw ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 30, M = 1, B = 16;
const double kMaxRisk = 0.2, kThreshold = 50.0, kMapMaxRisk = 0.5;  // (the solved plans all pass within 2 m of the obstacle: the safest read 0.08 and 0.15)


struct Scene {
  Parameters params;
  Matrix path{2, 200};
  std::vector<double> egos;
  std::vector<Obstacle> obstacles;
  Uncertainty um;
  double sigma0[16] = {}, W[16] = {};
};

// One configuration: the sequence by hand on a handle of its own, then a fresh planner.  Returns false (after saying why) on a mismatch.
bool run_case(const Scene& sc, const char* name, CandidatePick pick, bool sum_bound, bool with_map) {
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  const cilqr_uncertainty_map m = abi_map(sc.um);
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B), ok(B), mhits((size_t)B * N), munk((size_t)B * N);
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16}, zero[4] = {0.0, 0.0, 0.0, 0.0};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};  // one set for the batch, constant over the horizon
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), score((size_t)B * CILQR_SCORE_FIELDS), base(B);
  std::vector<double> risk((size_t)B * CILQR_CHANCE_FIELDS), step((size_t)B * N), total(B), none_total(B), mrisk((size_t)B * CILQR_MAP_RISK_FIELDS), mtotal(B);
  const bool scored = pick == CandidatePick::MinTotalCost;
  const uint32_t flags = sum_bound ? CILQR_CHANCE_BOUND_SUM : 0u;
  bool done = cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
              (!with_map || cilqr_set_uncertainty_map(h, &m) == CILQR_OK) &&
              cilqr_solve_batch_obstacles(h, B, N, M, sc.egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(),
                                          status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
              (!scored || cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, score.data(), base.data()) == CILQR_OK) &&
              cilqr_gains_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK;
  const double* rank = scored ? base.data() : J.data();
  done = done &&
         cilqr_chance_risk(h, B, N, M, X.data(), U.data(), K.data(), sc.sigma0, 0, sc.W, &obs, flags, -1.0, rank, risk.data(), nullptr, nullptr,
                           nullptr, none_total.data()) == CILQR_OK &&
         cilqr_chance_risk(h, B, N, M, X.data(), U.data(), K.data(), sc.sigma0, 0, sc.W, &obs, flags, kMaxRisk, rank, risk.data(), step.data(),
                           nullptr, nullptr, total.data()) == CILQR_OK &&
         (!with_map || cilqr_rollout_risk_map(h, B, N, 1, X.data(), U.data(), k.data(), K.data(), zero, 0, 0.0, kThreshold, 0u, kMapMaxRisk,
                                              total.data(), mrisk.data(), mhits.data(), munk.data(), mtotal.data()) == CILQR_OK);
  if (!done) { printf("%s: the sequence by hand failed: %s\n", name, cilqr_last_error()); return false; }
  cilqr_destroy(h);
  const std::vector<double>& final_total = with_map ? mtotal : total;
  const int want = first_minimum(final_total);
  int rejected = 0, by_map = 0;
  for (int b = 0; b < B; ++b) {
    rejected += total[b] != total[b];
    by_map += with_map && total[b] == total[b] && mtotal[b] != mtotal[b];
    const double* r = &risk[(size_t)CILQR_CHANCE_FIELDS * b];
    printf("%s candidate %2d: rank %.6f step risk %.6f (step %g) sum risk %.6f max p %.6f (entry %g) pos sigma %.4f%s\n", name, b, rank[b],
           r[CILQR_CR_STEP_RISK], r[CILQR_CR_WORST_STEP], r[CILQR_CR_SUM_RISK], r[CILQR_CR_MAX_P], r[CILQR_CR_MAX_ENTRY],
           r[CILQR_CR_MAX_POS_SIGMA], with_map && mtotal[b] != mtotal[b] && total[b] == total[b] ? "  rejected by the map" : "");
  }
  printf("%s: pick by hand among %s <= %g: %d; %d of %d candidates rejected by the chance value, %d more by the map\n", name,
         sum_bound ? "CR_SUM_RISK" : "CR_STEP_RISK", kMaxRisk, want, rejected, B, by_map);
  if (rejected == 0 || rejected == B || first_minimum(total) < 0 || first_minimum(none_total) != -1) {  // (the map may reject the rest: then -1 on both sides)
    printf("%s: the scene does not separate the candidates\n", name);
    return false;
  }

  iLQR planner(sc.params, 0, M, B);
  planner.set_global_plan(sc.path);
  planner.set_Obstacle(sc.obstacles);
  planner.set_candidate_pick(pick, 0.0);
  if (with_map) {
    planner.set_uncertainty_map(sc.um);
    planner.set_map_risk_check(kThreshold, kMapMaxRisk);
  }
  planner.set_pose_covariance_check(sc.sigma0, sc.W, kMaxRisk, 1.0, sum_bound);
  const int best = planner.run_candidates(sc.egos);
  if (best != want) { printf("%s: the check picked %d, the sequence by hand %d\n", name, best, want); return false; }
  if (best < 0) return planner.last_chance_risk.size() == risk.size() && same(planner.last_chance_risk.data(), risk.data(), risk.size());
  if (planner.last_chance_risk.size() != risk.size() || !same(planner.last_chance_risk.data(), risk.data(), risk.size()) ||
      planner.last_step_risk.size() != step.size() || !same(planner.last_step_risk.data(), step.data(), step.size())) {
    printf("%s: last_chance_risk / last_step_risk differ from cilqr_chance_risk on the same solves\n", name);
    return false;
  }
  if (scored ? planner.last_scores.size() != score.size() || !same(planner.last_scores.data(), score.data(), score.size())
             : !planner.last_scores.empty()) {
    printf("%s: last_scores differs from cilqr_score_batch on the same solves\n", name);
    return false;
  }
  if (with_map ? planner.last_map_risk.size() != mrisk.size() || !same(planner.last_map_risk.data(), mrisk.data(), mrisk.size()) ||
                     memcmp(planner.last_map_step_hits.data(), mhits.data(), mhits.size() * sizeof(int32_t)) != 0
               : !planner.last_map_risk.empty()) {
    printf("%s: last_map_risk differs from cilqr_rollout_risk_map on the same solves\n", name);
    return false;
  }
  if (!planner.last_risk.empty() || !planner.last_step_hits.empty()) { printf("%s: last_risk is not empty\n", name); return false; }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best]) {
    printf("%s: the pick's X / U / J differ from the hand-written solve\n", name);
    return false;
  }
  if (with_map || scored || sum_bound) return true;
  // 2. every candidate rejected
  const Matrix X_before = planner.X_result, U_before = planner.U_result;
  const double cost_before = planner.last_cost;
  planner.set_pose_covariance_check(sc.sigma0, sc.W, -1.0);
  if (planner.run_candidates(sc.egos) != -1) { printf("every candidate rejected, yet there is a pick\n"); return false; }
  if (!same(planner.U_result.a.data(), U_before.a.data(), U_before.a.size()) || !same(planner.X_result.a.data(), X_before.a.data(), X_before.a.size()) ||
      !same(&planner.last_cost, &cost_before, 1) || planner.last_chance_risk.size() != risk.size()) {
    printf("all rejected: results were touched\n");
    return false;
  }
  // 3. switched off: the default pick by J
  planner.set_pose_covariance_check(nullptr, nullptr, 1.0);
  const int plain = planner.run_candidates(sc.egos);
  if (plain < 0 || !planner.last_chance_risk.empty() || !planner.last_step_risk.empty()) { printf("check off: pick %d, last_chance_risk not empty\n", plain); return false; }
  return true;
}

// params.horizon changed after the setter, under the check: the block is laid out anew, and the run equals the sequence by hand at the
// new horizon N2 on a handle made as the planner's was, from the first N2 steps of the warm start the first run left.
bool horizon_case(const Scene& sc) {
  const int N2 = 12;
  iLQR planner(sc.params, 0, M, B);
  planner.set_global_plan(sc.path);
  planner.set_Obstacle(sc.obstacles);
  planner.set_pose_covariance_check(sc.sigma0, sc.W, kMaxRisk);
  if (planner.run_candidates(sc.egos) < 0) { printf("horizon: no pick at the first horizon\n"); return false; }
  const std::vector<double> warm(planner.U_result.a.begin(), planner.U_result.a.begin() + 2 * N2);

  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U((size_t)B * 2 * N2), X((size_t)B * 4 * (N2 + 1)), J(B);
  std::vector<double> k((size_t)B * 2 * N2), K((size_t)B * 8 * N2), risk((size_t)B * CILQR_CHANCE_FIELDS), step((size_t)B * N2), total(B);
  std::vector<int32_t> iters(B), status(B), ok(B);
  for (int b = 0; b < B; ++b) memcpy(&U[(size_t)b * 2 * N2], warm.data(), warm.size() * sizeof(double));
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};
  const bool done =
      cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_obstacles(h, B, N2, M, sc.egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(),
                                  status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch(h, B, N2, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_chance_risk(h, B, N2, M, X.data(), U.data(), K.data(), sc.sigma0, 0, sc.W, &obs, 0u, kMaxRisk, J.data(), risk.data(), step.data(),
                        nullptr, nullptr, total.data()) == CILQR_OK;
  if (!done) { printf("horizon: the sequence by hand failed: %s\n", cilqr_last_error()); return false; }
  cilqr_destroy(h);
  const int want = first_minimum(total);
  printf("horizon %d: pick by hand %d; %d of %d candidates rejected\n", N2, want, count_nan(total), B);
  if (want < 0) { printf("horizon: every candidate is rejected at the new horizon\n"); return false; }

  planner.params.horizon = N2;
  const int best = planner.run_candidates(sc.egos);
  if (best != want) { printf("horizon: the check picked %d, the sequence by hand %d\n", best, want); return false; }
  if (!same(planner.last_chance_risk, risk) || !same(planner.last_step_risk, step)) {
    printf("horizon: last_chance_risk / last_step_risk differ from cilqr_chance_risk at the new horizon\n");
    return false;
  }
  if (planner.X_result.cols != N2 + 1 || !same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N2 + 1)], 4 * (size_t)(N2 + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N2], 2 * (size_t)N2) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best]) {
    printf("horizon: the pick's X / U / J differ from the hand-written solve at the new horizon\n");
    return false;
  }
  return true;
}
}  // namespace

int main() {
  Scene sc;
  sc.params = default_parameters();
  sc.params.horizon = N;
  sc.path = straight_path();
  sc.egos = spread_egos(B, -3.0, 0.5);
  sc.obstacles = {standing_obstacle(sc.params, N, 12.0, -1.0)};
  sc.sigma0[0] = 0.16 * 0.16; sc.sigma0[5] = 0.16 * 0.16; sc.sigma0[15] = 0.017 * 0.017;
  sc.W[0] = 1e-4; sc.W[5] = 1e-4; sc.W[10] = 4e-4; sc.W[15] = 1e-6;
  // the costmap: 200 x 80 cells of 0.2 m centred 15 m ahead; cell (i, j) has its centre at (34.9 - 0.2 i, 7.9 - 0.2 j); a smooth
  // occupied region around (20, 3.5), where candidates far from the obstacle drive
  if (!bump_costmap(sc.um, {{90.0, 20.0, 3.5, 5.0, 0.7}})) return 1;

  if (!run_case(sc, "J", CandidatePick::MinTrackingCost, false, false)) return 1;
  if (!run_case(sc, "total", CandidatePick::MinTotalCost, false, false)) return 1;
  if (!run_case(sc, "sum", CandidatePick::MinTrackingCost, true, false)) return 1;
  if (!run_case(sc, "map", CandidatePick::MinTotalCost, false, true)) return 1;
  if (!horizon_case(sc)) return 1;
  printf("chance pick ok\n");

  // 4. the conflicts, in both orders
  const std::vector<double> offsets(8, 0.01), samples(3 * 2, 0.05);
  {
    iLQR p(sc.params, 0, 4, B);
    p.set_pose_covariance_check(sc.sigma0, nullptr, 0.05);
    if (!throws_logic_error([&] { p.set_pose_noise_check_fused(offsets, 0.1); }, "set_pose_covariance_check") ||
        !throws_logic_error([&] { p.set_pose_noise_check(offsets, 0.1); }, "set_pose_covariance_check") ||
        !throws_logic_error([&] { p.set_obstacle_samples(samples, 2); }, "set_obstacle_samples")) {
      printf("a noise or sample setter after set_pose_covariance_check did not throw std::logic_error naming the conflict\n");
      return 1;
    }
    p.set_pose_noise_check_fused({}, 1.0);  // (switching the draws off is no conflict)
  }
  {
    iLQR p(sc.params, 0, 4, B);
    p.set_pose_noise_check_fused(offsets, 0.1);
    if (!throws_logic_error([&] { p.set_pose_covariance_check(sc.sigma0, nullptr, 0.05); }, "set_pose_noise_check")) {
      printf("set_pose_covariance_check after set_pose_noise_check_fused did not throw\n");
      return 1;
    }
    p.set_pose_noise_check_fused({}, 1.0);
    p.set_obstacle_samples(samples, 2);
    if (!throws_logic_error([&] { p.set_pose_covariance_check(sc.sigma0, nullptr, 0.05); }, "set_obstacle_samples")) {
      printf("set_pose_covariance_check after set_obstacle_samples did not throw\n");
      return 1;
    }
    p.set_pose_covariance_check(nullptr, nullptr, 1.0);  // (off: no conflict)
  }
  printf("conflicts throw ok\n");
  return 0;
}
