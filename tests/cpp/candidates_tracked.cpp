// candidates_tracked.cpp — iLQR::set_tracked_obstacles and iLQR::set_obstacle_covariance_check: a straight path, four candidates
// at y = 0, 0.3, 0.6, 0.9 m and 5 m/s, ONE oncoming tracked vehicle (30, 3.4, 5, pi, 0, 0), 4 x 2 m, with the tracker covariance
// P_0 = diag(0.3^2, 0.3^2, 0.5^2, 0.05^2) and Q = diag(1e-4, 1e-4, 4e-4, 1e-6); the node's pose noise as Sigma0 =
// diag(0.16^2, 0.16^2, 0, 0.017^2) with that Q as process noise.  The cheapest candidate (on the path) is the riskiest.
//   usage: candidates_tracked MAX_RISK PICK_OFF PICK_ON   (the picks expected with the check off and on: the caller's CPU figures)
//   1. set_tracked_obstacles against the table cilqr_predict_obstacles gives by hand, installed with set_Obstacle +
//      set_obstacle_covariance (3 * M * N form): the same pick, X_result, U_result, last_cost and last_chance_risk, bit for bit, with
//      the check off and on;
//   2. check off: those results are, bit for bit, the ones of a planner that got set_Obstacle alone — no covariance, neither new call;
//   3. check on: last_chance_risk and last_step_risk are cilqr_chance_risk_cov's on the C-ABI sequence called by hand (local plan,
//      solve, gains, chance risk with obs_cov), the pick is its strict-< first minimum, and it is PICK_ON != PICK_OFF;
//   4. params.horizon changed after set_tracked_obstacles: the vehicles are predicted again (equal to the hand-built table of the new
//      horizon, 28); clear_Obstacle removes obstacles and covariance (every CR_STEP_RISK is 0).
// Prints the candidates' figures with their margins to MAX_RISK, then "tracked equals hand-built ok", "check off is the parent ok",
// "check changes the pick ok", "horizon change and clear ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 30, M = 1, B = 4;


struct Scene {
  Parameters params;
  Matrix path{2, 200};
  std::vector<double> egos, tracks, dims, P0, Q;
  double sigma0[16] = {}, W[16] = {};
};

struct Result {
  int pick;
  Matrix X, U;
  double cost;
  std::vector<double> risk, step;
};
Result run(iLQR& p, const Scene& sc) {
  Result r;
  r.pick = p.run_candidates(sc.egos);
  r.X = p.X_result; r.U = p.U_result; r.cost = p.last_cost; r.risk = p.last_chance_risk; r.step = p.last_step_risk;
  return r;
}
bool equal(const Result& a, const Result& b) {
  return a.pick == b.pick && same(a.X.a, b.X.a) && same(a.U.a, b.U.a) && same(&a.cost, &b.cost, 1) && same(a.risk, b.risk) && same(a.step, b.step);
}

// The predicted table by hand, on a handle of its own.
bool predict_by_hand(const Scene& sc, int horizon, std::vector<double>& pose, std::vector<double>& dim, std::vector<double>& cov) {
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, B, N, M, 0, &h) != CILQR_OK) return false;
  pose.assign((size_t)M * 4 * horizon, 0.0); dim.assign((size_t)M * 2 * horizon, 0.0); cov.assign((size_t)M * 3 * horizon, 0.0);
  const int rc = cilqr_predict_obstacles(h, 1, horizon, M, sc.tracks.data(), sc.dims.data(), sc.P0.data(), sc.Q.data(), pose.data(), dim.data(),
                                         cov.data(), nullptr);
  cilqr_destroy(h);
  return rc == CILQR_OK;
}
std::vector<Obstacle> obstacles_of(const Scene& sc, int horizon, const std::vector<double>& pose, const std::vector<double>& dim) {
  std::vector<Obstacle> out;
  for (int m = 0; m < M; ++m) {
    Matrix d(2, horizon), r(4, horizon);
    memcpy(d.a.data(), &dim[(size_t)m * 2 * horizon], (size_t)2 * horizon * sizeof(double));
    memcpy(r.a.data(), &pose[(size_t)m * 4 * horizon], (size_t)4 * horizon * sizeof(double));
    out.emplace_back(sc.params, d, r);
  }
  return out;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { printf("usage: candidates_tracked MAX_RISK PICK_OFF PICK_ON\n"); return 2; }
  const double max_risk = atof(argv[1]);
  const int want_off = atoi(argv[2]), want_on = atoi(argv[3]);
  Scene sc;
  sc.params = default_parameters();
  sc.params.horizon = N;
  sc.path = straight_path();
  for (int b = 0; b < B; ++b) { const double e[4] = {0.0, 0.3 * b, 5.0, 0.0}; sc.egos.insert(sc.egos.end(), e, e + 4); }
  sc.tracks = {30.0, 3.4, 5.0, 3.14159265358979311600, 0.0, 0.0};
  sc.dims = {4.0, 2.0};
  sc.P0.assign(16, 0.0);
  sc.P0[0] = 0.3 * 0.3; sc.P0[5] = 0.3 * 0.3; sc.P0[10] = 0.5 * 0.5; sc.P0[15] = 0.05 * 0.05;
  sc.Q.assign(16, 0.0);
  sc.Q[0] = 1e-4; sc.Q[5] = 1e-4; sc.Q[10] = 4e-4; sc.Q[15] = 1e-6;
  sc.sigma0[0] = 0.16 * 0.16; sc.sigma0[5] = 0.16 * 0.16; sc.sigma0[15] = 0.017 * 0.017;
  memcpy(sc.W, sc.Q.data(), sizeof(sc.W));

  std::vector<double> pose, dim, cov;
  if (!predict_by_hand(sc, N, pose, dim, cov)) { printf("cilqr_predict_obstacles by hand failed: %s\n", cilqr_last_error()); return 1; }

  // ---- 1, 2: tracked against hand-built against the planner that knows neither new call
  iLQR tracked(sc.params, 0, M, B), built(sc.params, 0, M, B), parent(sc.params, 0, M, B);
  for (iLQR* p : {&tracked, &built, &parent}) {
    p->set_global_plan(sc.path);
    p->set_pose_covariance_check(sc.sigma0, sc.W, max_risk);
  }
  tracked.set_tracked_obstacles(sc.tracks, sc.dims, sc.P0, sc.Q);
  built.set_Obstacle(obstacles_of(sc, N, pose, dim));
  built.set_obstacle_covariance(cov);
  parent.set_Obstacle(obstacles_of(sc, N, pose, dim));
  const Result t_off = run(tracked, sc), b_off = run(built, sc), p_off = run(parent, sc);
  if (!equal(t_off, b_off)) { printf("check off: set_tracked_obstacles differs from set_Obstacle + set_obstacle_covariance (picks %d, %d)\n", t_off.pick, b_off.pick); return 1; }
  if (!equal(t_off, p_off)) { printf("check off: the results differ from a planner without the covariance (picks %d, %d)\n", t_off.pick, p_off.pick); return 1; }

  // ---- 3: the sequence by hand with obs_cov, from the default warm start the planners started from
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B), ok(B);
  const cilqr_obstacles obs{pose.data(), dim.data(), nullptr, 0, N, 1, 0};  // one predicted set for every candidate
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), risk((size_t)B * CILQR_CHANCE_FIELDS), step((size_t)B * N), total(B),
      bare((size_t)B * CILQR_CHANCE_FIELDS), bare_total(B);
  const bool done =
      cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_obstacles(h, B, N, M, sc.egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(), status.data(),
                                  CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_chance_risk_cov(h, B, N, M, X.data(), U.data(), K.data(), sc.sigma0, 0, sc.W, &obs, cov.data(), 0u, max_risk, J.data(), risk.data(),
                            step.data(), nullptr, nullptr, total.data()) == CILQR_OK &&
      cilqr_chance_risk(h, B, N, M, X.data(), U.data(), K.data(), sc.sigma0, 0, sc.W, &obs, 0u, max_risk, J.data(), bare.data(), nullptr, nullptr,
                        nullptr, bare_total.data()) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  cilqr_destroy(h);
  for (int b = 0; b < B; ++b)
    printf("candidate %d: J %.9f  CR_STEP_RISK with the covariance %.12g (margin to %.4g: %+.3e)  without %.6g\n", b, J[b],
           risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK], max_risk, risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK] - max_risk,
           bare[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK]);
  if (!same(t_off.risk, bare) || t_off.pick != first_minimum(bare_total)) { printf("check off: last_chance_risk is not cilqr_chance_risk's by hand\n"); return 1; }
  printf("tracked equals hand-built ok\ncheck off is the parent ok\n");

  // (fresh planners: run_candidates keeps the pick as the next warm start)
  iLQR tracked_on(sc.params, 0, M, B), built_on(sc.params, 0, M, B);
  for (iLQR* p : {&tracked_on, &built_on}) {
    p->set_global_plan(sc.path);
    p->set_obstacle_covariance_check(true);
    p->set_pose_covariance_check(sc.sigma0, sc.W, max_risk);
  }
  tracked_on.set_tracked_obstacles(sc.tracks, sc.dims, sc.P0, sc.Q);
  built_on.set_Obstacle(obstacles_of(sc, N, pose, dim));
  built_on.set_obstacle_covariance(cov);
  const Result t_on = run(tracked_on, sc), b_on = run(built_on, sc);
  if (!equal(t_on, b_on)) { printf("check on: set_tracked_obstacles differs from the hand-built form (picks %d, %d)\n", t_on.pick, b_on.pick); return 1; }
  const int by_hand = first_minimum(total);
  if (!same(t_on.risk, risk) || !same(t_on.step, step) || t_on.pick != by_hand) { printf("check on: pick %d, by hand %d, or the risk rows differ from cilqr_chance_risk_cov\n", t_on.pick, by_hand); return 1; }
  if (t_on.pick < 0 || !same(t_on.X.a.data(), &X[(size_t)t_on.pick * 4 * (N + 1)], 4 * (size_t)(N + 1)) || !same(&t_on.cost, &J[t_on.pick], 1)) { printf("check on: the pick's plan differs from the solve by hand\n"); return 1; }
  printf("pick with the check off %d (expected %d), on %d (expected %d)\n", t_off.pick, want_off, t_on.pick, want_on);
  if (t_off.pick != want_off || t_on.pick != want_on || t_on.pick == t_off.pick) { printf("the picks are not the expected ones\n"); return 1; }
  // the check switched on by the setter AFTER the covariance check, and off again
  parent.set_obstacle_covariance(cov);
  parent.set_obstacle_covariance_check(true);
  parent.set_obstacle_covariance_check(false);
  built.set_obstacle_covariance_check(true);
  built.set_obstacle_covariance_check(false);
  if (!equal(run(parent, sc), run(built, sc))) { printf("switching the check on and off again left something behind\n"); return 1; }
  printf("check changes the pick ok\n");

  // ---- 4: the horizon changes after set_tracked_obstacles; clear_Obstacle
  const int N2 = 28;
  std::vector<double> pose2, dim2, cov2;
  if (!predict_by_hand(sc, N2, pose2, dim2, cov2)) { printf("cilqr_predict_obstacles by hand failed: %s\n", cilqr_last_error()); return 1; }
  iLQR tracked2(sc.params, 0, M, B), built2(sc.params, 0, M, B);
  for (iLQR* p : {&tracked2, &built2}) {
    p->set_global_plan(sc.path);
    p->set_obstacle_covariance_check(true);
    p->set_pose_covariance_check(sc.sigma0, sc.W, max_risk);
  }
  tracked2.set_tracked_obstacles(sc.tracks, sc.dims, sc.P0, sc.Q);  // predicted over 30 steps here
  tracked2.params.horizon = N2;
  built2.params.horizon = N2;
  built2.set_Obstacle(obstacles_of(sc, N2, pose2, dim2));
  built2.set_obstacle_covariance(cov2);
  const Result t2 = run(tracked2, sc), b2 = run(built2, sc);
  if (t2.X.cols != N2 + 1 || !equal(t2, b2)) { printf("after a horizon change the tracked planner differs from the hand-built one (picks %d, %d)\n", t2.pick, b2.pick); return 1; }
  // (a stale 30-step covariance would not match the 20-step table: the run above would have thrown)
  for (int b = 0; b < B; ++b) printf("horizon %d, candidate %d: CR_STEP_RISK %.6g\n", N2, b, t2.risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK]);
  tracked2.clear_Obstacle();
  const Result cleared = run(tracked2, sc);
  for (int b = 0; b < B; ++b)
    if (cleared.risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK] != 0.0 || cleared.risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_WORST_STEP] != -1.0) {
      printf("clear_Obstacle left an obstacle behind\n");
      return 1;
    }
  printf("horizon change and clear ok\n");
  return 0;
}
