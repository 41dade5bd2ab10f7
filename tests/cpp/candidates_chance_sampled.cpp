// candidates_chance_sampled.cpp — iLQR::set_sample_covariance_check: four candidates beside a straight path, one nominal obstacle
// 2.5 m to its right with 8 pose samples (sigma 0.45 m, 0.05 rad) shared by the candidates (the scene of candidates_risk_sampled.cpp),
// Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2), no process noise.
//   1. with samples set, run_candidates under set_sample_covariance_check returns the index the C-ABI sequence called by hand gives —
//      cilqr_solve_batch_sampled, cilqr_gains_batch_sampled(lamb 1), cilqr_score_batch_sampled (nominal totals, max_collision 1),
//      cilqr_chance_risk (M = 0, sigma_out, base = those totals), cilqr_chance_risk_sampled (base = that total), strict-< first minimum
//      of its `total` — with X_result / U_result / last_cost of that candidate, and last_chance_risk_sampled (CILQR_CRS_FIELDS per
//      candidate) and last_scores equal to that sequence's, bit for bit.  max_risk lies midway between the two largest CRS_STEP_RISK
//      of the candidates (which must be more than 1e-6 apart): it rejects at least one candidate and not all;
//   2. a max_risk below every chance (-1) rejects all: the index is -1 and the results stay;
//   3. together with set_pose_noise_check(_fused) offsets whichever comes second throws std::logic_error naming the other setter;
//      without samples set run_candidates throws std::logic_error naming set_pose_covariance_check; and set_pose_covariance_check
//      with samples set still throws std::logic_error;
//   4. one planner switched fused check -> sample covariance check -> fused check -> sample covariance check: a field the mode in force
//      does not produce is empty, and every run equals a run from the same warm start on a planner that never switched.
// Prints "sample chance pick ok", "rejects all ok", "conflicts throw ok" and "mode switches ok" on success.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 30, n_obs = 1, ns = 8, M = n_obs * ns, B = 4, S = 70;
  const int F = CILQR_CRS_FIELDS;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, 0.0, 0.6);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 12.0, -2.5)};
  Draws draws;
  const std::vector<double> offsets = make_offsets(S, draws), samples = make_pose_samples(n_obs * ns, draws);
  const double weight = params.w_obstacle / ns;
  double sigma0[16] = {};
  sigma0[0] = 0.16 * 0.16; sigma0[5] = 0.16 * 0.16; sigma0[15] = 0.017 * 0.017;

  // by hand: the host-buffer forms, the obstacle set repeated for every candidate
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B), ok(B);
  std::vector<double> nom_pose((size_t)B * n_obs * 4 * N), nom_dim((size_t)B * n_obs * 2 * N), off((size_t)B * samples.size());
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < N; ++t) {
      for (int r = 0; r < 4; ++r) nom_pose[((size_t)b * N + t) * 4 + r] = obstacles[0].relative_pos_array(r, t);
      for (int r = 0; r < 2; ++r) nom_dim[((size_t)b * N + t) * 2 + r] = obstacles[0].dimension(r, t);
    }
    memcpy(&off[(size_t)b * samples.size()], samples.data(), samples.size() * sizeof(double));
  }
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), score((size_t)B * CILQR_SCORE_FIELDS), base(B);
  std::vector<double> crisk((size_t)B * CILQR_CHANCE_FIELDS), sigma((size_t)B * (N + 1) * 16), ctotal(B), risk((size_t)B * F), total(B);
  bool done =
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_sampled(h, B, N, n_obs, ns, egos.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, X.data(), J.data(), iters.data(), status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch_sampled(h, B, N, n_obs, ns, X.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_score_batch_sampled(h, B, N, n_obs, ns, X.data(), U.data(), poly.data(), fl.data(), nom_pose.data(), nom_dim.data(), off.data(),
                                weight, 1.0, score.data(), base.data()) == CILQR_OK &&
      // (first with max_risk 1: the candidates' figures, from which the bound is taken)
      cilqr_chance_risk(h, B, N, 0, X.data(), U.data(), K.data(), sigma0, 0, nullptr, nullptr, 0u, 1.0, base.data(), crisk.data(), nullptr,
                        nullptr, sigma.data(), ctotal.data()) == CILQR_OK &&
      cilqr_chance_risk_sampled(h, B, N, n_obs, ns, X.data(), sigma.data(), nom_pose.data(), nom_dim.data(), off.data(), 0u, 1.0, ctotal.data(),
                                risk.data(), nullptr, nullptr, nullptr, total.data()) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> r(B);
  for (int b = 0; b < B; ++b) {
    const double* f = &risk[(size_t)F * b];
    r[b] = f[CILQR_CRS_STEP_RISK];
    printf("candidate %d: nominal total %.6f step risk %.6f (step %g) sum %.6f max pair p %.6f max entry p %.6f nominal share %.4f\n", b, base[b],
           f[CILQR_CRS_STEP_RISK], f[CILQR_CRS_WORST_STEP], f[CILQR_CRS_SUM_RISK], f[CILQR_CRS_MAX_PAIR_P], f[CILQR_CRS_MAX_ENTRY_P],
           f[CILQR_CRS_NOMINAL_SHARE]);
  }
  std::sort(r.begin(), r.end());
  if (!(r[B - 1] - r[B - 2] > 1e-6)) { printf("the scene does not separate the candidates by risk\n"); return 1; }
  const double max_risk = 0.5 * (r[B - 1] + r[B - 2]);
  done = cilqr_chance_risk(h, B, N, 0, X.data(), U.data(), K.data(), sigma0, 0, nullptr, nullptr, 0u, max_risk, base.data(), crisk.data(),
                           nullptr, nullptr, sigma.data(), ctotal.data()) == CILQR_OK &&
         cilqr_chance_risk_sampled(h, B, N, n_obs, ns, X.data(), sigma.data(), nom_pose.data(), nom_dim.data(), off.data(), 0u, max_risk,
                                   ctotal.data(), risk.data(), nullptr, nullptr, nullptr, total.data()) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  cilqr_destroy(h);
  const int want = first_minimum(total);
  int rejected = 0;
  for (int b = 0; b < B; ++b) rejected += total[b] != total[b];
  printf("pick by hand: nominal total among step risk <= %.6f: %d; %d of %d candidates rejected\n", max_risk, want, rejected, B);
  if (rejected == 0 || rejected == B || want < 0) { printf("the bound does not separate the candidates\n"); return 1; }

  // 1. the check with samples set
  iLQR planner(params, 0, M, B);
  planner.set_global_plan(path);
  planner.set_Obstacle(obstacles);
  planner.set_obstacle_samples(samples, ns);
  planner.set_sample_covariance_check(sigma0, nullptr, max_risk);
  const int best = planner.run_candidates(egos);
  if (best != want) { printf("the check picked %d, the sequence by hand %d\n", best, want); return 1; }
  if (!same(planner.last_chance_risk_sampled, risk)) { printf("last_chance_risk_sampled differs from cilqr_chance_risk_sampled on the same solves\n"); return 1; }
  if (!same(planner.last_scores, score)) { printf("last_scores differs from cilqr_score_batch_sampled on the same solves\n"); return 1; }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best]) {
    printf("the pick's X / U / J differ from the hand-written solve\n");
    return 1;
  }
  printf("sample chance pick ok\n");

  // 2. a bound below every chance rejects all
  {
    iLQR q(params, 0, M, B);
    q.set_global_plan(path);
    q.set_Obstacle(obstacles);
    q.set_obstacle_samples(samples, ns);
    q.set_sample_covariance_check(sigma0, nullptr, -1.0);
    const int none = q.run_candidates(egos);
    if (none != -1 || q.last_chance_risk_sampled.size() != (size_t)B * F || !same(q.last_chance_risk_sampled, risk)) {
      printf("max_risk -1: pick %d, not -1\n", none);
      return 1;
    }
    printf("rejects all ok\n");
  }

  // 3. the conflicts
  {
    iLQR a(params, 0, M, B);
    a.set_global_plan(path);
    a.set_Obstacle(obstacles);
    a.set_obstacle_samples(samples, ns);
    a.set_sample_covariance_check(sigma0, nullptr, 0.1);
    if (!throws_logic_error([&] { a.set_pose_noise_check_fused(offsets, 0.1); }, "set_sample_covariance_check")) {
      printf("set_pose_noise_check_fused after set_sample_covariance_check did not throw std::logic_error naming it\n");
      return 1;
    }
    if (!throws_logic_error([&] { a.set_pose_covariance_check(sigma0, nullptr, 0.1); }, "set_obstacle_samples")) {
      printf("set_pose_covariance_check with samples set did not throw std::logic_error\n");
      return 1;
    }
    iLQR b(params, 0, M, B);
    b.set_global_plan(path);
    b.set_Obstacle(obstacles);
    b.set_obstacle_samples(samples, ns);
    b.set_pose_noise_check_fused(offsets, 0.1);
    if (!throws_logic_error([&] { b.set_sample_covariance_check(sigma0, nullptr, 0.1); }, "set_pose_noise_check")) {
      printf("set_sample_covariance_check after a noise setter did not throw std::logic_error naming it\n");
      return 1;
    }
    iLQR c(params, 0, M, B);
    c.set_global_plan(path);
    c.set_Obstacle(obstacles);
    c.set_sample_covariance_check(sigma0, nullptr, 0.1);
    // (the stored-rows setter: on a planner without samples, where its own conflict with them does not come first)
    if (!throws_logic_error([&] { c.set_pose_noise_check(offsets, 0.1); }, "set_sample_covariance_check")) {
      printf("set_pose_noise_check after set_sample_covariance_check did not throw std::logic_error naming it\n");
      return 1;
    }
    if (!throws_logic_error([&] { c.run_candidates(egos); }, "set_pose_covariance_check")) {
      printf("run_candidates under set_sample_covariance_check without samples did not throw std::logic_error naming set_pose_covariance_check\n");
      return 1;
    }
    printf("conflicts throw ok\n");
  }

  // 4. one planner across mode switches, in the one device block: fused check -> sample covariance check -> fused check -> sample
  //    covariance check.  The first three runs reject every candidate (max_risk -1), so the warm start stays the fresh planner's and
  //    each run can be held against a run from that start: the planner of 2. (its rows are `risk`), the first run, the planner of 1.
  {
    iLQR a(params, 0, M, B);
    a.set_global_plan(path);
    a.set_Obstacle(obstacles);
    a.set_obstacle_samples(samples, ns);
    a.set_pose_noise_check_fused(offsets, -1.0);
    if (a.run_candidates(egos) != -1 || a.last_risk.size() != (size_t)B * CILQR_RRS_FIELDS || a.last_step_hits.size() != (size_t)B * N ||
        !same(a.last_scores, score) || !a.last_chance_risk_sampled.empty()) {
      printf("mode switches: the fused run\n");
      return 1;
    }
    const std::vector<double> risk1 = a.last_risk;
    const std::vector<int32_t> hits1 = a.last_step_hits;
    a.set_pose_noise_check_fused({}, 1.0);
    a.set_sample_covariance_check(sigma0, nullptr, -1.0);
    if (a.run_candidates(egos) != -1) { printf("mode switches: max_risk -1 under the sample covariance check gave a pick\n"); return 1; }
    if (!a.last_risk.empty() || !a.last_step_hits.empty()) {
      printf("mode switches: last_risk / last_step_hits are not empty under the sample covariance check\n");
      return 1;
    }
    if (!same(a.last_chance_risk_sampled, risk) || !same(a.last_scores, score)) {
      printf("mode switches: last_chance_risk_sampled differs from a fresh planner's\n");
      return 1;
    }
    a.set_sample_covariance_check(nullptr, nullptr, 1.0);
    a.set_pose_noise_check_fused(offsets, -1.0);
    if (a.run_candidates(egos) != -1 || !same(a.last_risk, risk1) || !same_i(a.last_step_hits, hits1) || !same(a.last_scores, score) ||
        !a.last_chance_risk_sampled.empty()) {
      printf("mode switches: the fused run after the sample covariance check differs from the one before it\n");
      return 1;
    }
    a.set_pose_noise_check_fused({}, 1.0);
    a.set_sample_covariance_check(sigma0, nullptr, max_risk);
    if (a.run_candidates(egos) != best || !same(a.last_chance_risk_sampled, planner.last_chance_risk_sampled) ||
        !same(a.last_scores, planner.last_scores) || !a.last_risk.empty() || !a.last_step_hits.empty() ||
        !same(a.X_result.a, planner.X_result.a) || !same(a.U_result.a, planner.U_result.a) || !same(&a.last_cost, &planner.last_cost, 1) ||
        a.last_iterations != planner.last_iterations || a.last_exit != planner.last_exit) {
      printf("mode switches: the pick differs from a fresh planner's\n");
      return 1;
    }
    printf("mode switches ok\n");
  }
  return 0;
}
