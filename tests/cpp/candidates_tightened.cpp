// candidates_tightened.cpp — iLQR::run_candidates and run_step under chance-constraint tightening (set_chance_tightening): the scene of
// candidates_chance.cpp, one static obstacle 1 m beside a straight path and candidates spread laterally across it, with the node's
// pose noise as a covariance, Sigma0 = diag(0.16^2, 0.16^2, 0, 0.017^2), and a small process noise.
//   1. with the tightening set, run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_solve_batch_obstacles,
//      then `rounds` times cilqr_gains_batch(lamb 1), cilqr_chance_risk (sigma_out), cilqr_tighten_obstacles(kappa of eps, max_inflate),
//      cilqr_solve_batch_obstacles on (pose_out, dim_out) from the U before; then the pick: strict-< first minimum of J, or under
//      MinTotalCost of cilqr_score_batch's total against the ORIGINAL obstacle — with X_result / U_result / last_cost / last_iterations
//      / last_exit of that candidate and last_tighten, last_tighten_risk_before equal to that sequence's, bit for bit; one round and
//      two, with and without set_obstacle_covariance;
//   2. composed with set_pose_covariance_check: the check's gains and chance risk run on the FINAL plan against the original obstacle,
//      and last_chance_risk is that call's; and with the stored-rows check (set_pose_noise_check): cilqr_gains_batch, cilqr_rollout_batch
//      and cilqr_score_rollouts on the final plans against the original obstacle, last_risk that call's;
//   3. run_step: the same sequence at B = 1 behind cilqr_local_plan;
//   4. rounds = 0 and Sigma0 == nullptr switch it off: the plain pick, empty last_tighten;
//   5. together with set_obstacle_samples, whichever comes second throws std::logic_error.
// Prints "tightened pick ok", "composed pick ok", "run_step ok", "off switches ok" and "conflicts throw ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 30, M = 1;
const double kEps = 0.05, kCap = 2.0, kMaxRisk = 0.2;
const double kPose[4] = {12.0, -1.0, 0.0, 0.0}, kDim[2] = {4.79, 2.16}, kCov[3] = {0.09, 0.01, 0.04};


struct Scene {
  Parameters params;
  Matrix path{2, 200};
  std::vector<double> egos;
  std::vector<Obstacle> obstacles;
  double sigma0[16] = {}, W[16] = {};
};

// The sequence by hand for B solves whose path fit is given; everything it leaves.
struct Hand {
  std::vector<double> U, X, J, U_first, tg, risk_before, K, k;
  std::vector<int32_t> iters, status;
};

bool by_hand(cilqr_handle* h, const Scene& sc, int B, const double* egos, const double* poly, const double* fl, int rounds, bool with_cov, Hand& o) {
  o.U = default_controls(B, N); o.X.assign((size_t)B * 4 * (N + 1), 0.0); o.J.assign(B, 0.0);
  o.iters.assign(B, 0); o.status.assign(B, 0);
  o.k.assign((size_t)B * 2 * N, 0.0); o.K.assign((size_t)B * 8 * N, 0.0);
  o.tg.assign((size_t)B * CILQR_TIGHTEN_FIELDS, 0.0); o.risk_before.assign(B, 0.0);
  std::vector<double> risk((size_t)B * CILQR_CHANCE_FIELDS), sigma((size_t)B * (N + 1) * 16);
  std::vector<double> tpose((size_t)B * M * 4 * N), tdim((size_t)B * M * 2 * N);
  std::vector<int32_t> ok(B);
  const cilqr_obstacles obs{kPose, kDim, nullptr, 0, 1, 0, 0};  // one set for the batch, constant over the horizon
  const cilqr_obstacles inflated{tpose.data(), tdim.data(), nullptr, (int64_t)M * N, N, 1, 0};
  const double kappa = cilqr_chance_kappa(kEps);
  bool done = cilqr_solve_batch_obstacles(h, B, N, M, egos, o.U.data(), poly, fl, &obs, o.X.data(), o.J.data(), o.iters.data(), o.status.data(),
                                          CILQR_FLAG_NONE) == CILQR_OK;
  o.U_first = o.U;
  for (int r = 0; r < rounds && done; ++r) {
    done = cilqr_gains_batch(h, B, N, M, o.X.data(), o.U.data(), poly, fl, &obs, 1.0, o.k.data(), o.K.data(), ok.data()) == CILQR_OK &&
           cilqr_chance_risk(h, B, N, M, o.X.data(), o.U.data(), o.K.data(), sc.sigma0, 0, sc.W, &obs, 0u, 1.0, nullptr, risk.data(), nullptr, nullptr,
                             sigma.data(), nullptr) == CILQR_OK &&
           cilqr_tighten_obstacles(h, B, N, M, o.X.data(), sigma.data(), &obs, with_cov ? kCov : nullptr, kappa, kCap, tpose.data(), tdim.data(),
                                   o.tg.data()) == CILQR_OK &&
           cilqr_solve_batch_obstacles(h, B, N, M, egos, o.U.data(), poly, fl, &inflated, o.X.data(), o.J.data(), o.iters.data(), o.status.data(),
                                       CILQR_FLAG_NONE) == CILQR_OK;
    for (int b = 0; b < B; ++b) o.risk_before[b] = risk[(size_t)b * CILQR_CHANCE_FIELDS + CILQR_CR_STEP_RISK];
  }
  if (!done) printf("the sequence by hand failed: %s\n", cilqr_last_error());
  return done;
}

bool results_match(const char* name, const iLQR& p, const Hand& o, int B, int best) {
  if (p.last_tighten.size() != o.tg.size() || !same(p.last_tighten.data(), o.tg.data(), o.tg.size()) ||
      p.last_tighten_risk_before.size() != (size_t)B || !same(p.last_tighten_risk_before.data(), o.risk_before.data(), B)) {
    printf("%s: last_tighten / last_tighten_risk_before differ from the sequence by hand\n", name);
    return false;
  }
  if (!same(p.X_result.a.data(), &o.X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(p.U_result.a.data(), &o.U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&p.last_cost, &o.J[best], 1) ||
      p.last_iterations != o.iters[best] || p.last_exit != o.status[best]) {
    printf("%s: the pick's X / U / J / iterations differ from the hand-written re-solve\n", name);
    return false;
  }
  return true;
}

// One configuration of run_candidates: by hand on a handle of its own, then a fresh planner.
bool run_case(const Scene& sc, const char* name, int B, CandidatePick pick, int rounds, bool with_cov, bool with_check) {
  cilqr_handle* h = nullptr;
  // (three times the batch: the host forms of cilqr_chance_risk with sigma_out and of cilqr_tighten_obstacles promise B <= max_batch / 2
  // and B <= 2 max_batch / 5; a solve's bits do not depend on the handle's max_batch)
  if (cilqr_create(&sc.params, 3 * B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2);
  Hand o;
  const cilqr_obstacles obs{kPose, kDim, nullptr, 0, 1, 0, 0};
  const bool scored = pick == CandidatePick::MinTotalCost;
  std::vector<double> score((size_t)B * CILQR_SCORE_FIELDS), total(B), crisk((size_t)B * CILQR_CHANCE_FIELDS), cstep((size_t)B * N);
  std::vector<int32_t> ok(B);
  bool done = cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
              by_hand(h, sc, B, sc.egos.data(), poly.data(), fl.data(), rounds, with_cov, o);
  // what follows judges the final plan against the ORIGINAL obstacle
  if (done && with_check) {
    done = (!scored || cilqr_score_batch(h, B, N, M, o.X.data(), o.U.data(), poly.data(), fl.data(), &obs, 1.0, score.data(), total.data()) == CILQR_OK) &&
           cilqr_gains_batch(h, B, N, M, o.X.data(), o.U.data(), poly.data(), fl.data(), &obs, 1.0, o.k.data(), o.K.data(), ok.data()) == CILQR_OK;
    const std::vector<double> base = scored ? total : o.J;
    done = done && cilqr_chance_risk(h, B, N, M, o.X.data(), o.U.data(), o.K.data(), sc.sigma0, 0, sc.W, &obs, 0u, kMaxRisk, base.data(), crisk.data(),
                                     cstep.data(), nullptr, nullptr, total.data()) == CILQR_OK;
  } else if (done && scored) {
    done = cilqr_score_batch(h, B, N, M, o.X.data(), o.U.data(), poly.data(), fl.data(), &obs, 0.0, score.data(), total.data()) == CILQR_OK;
  }
  if (!done) { printf("%s: the sequence by hand failed: %s\n", name, cilqr_last_error()); return false; }
  cilqr_destroy(h);
  const int want = first_minimum(with_check || scored ? total : o.J);
  double moved = 0.0;
  for (size_t i = 0; i < o.U.size(); ++i) moved = std::fmax(moved, std::fabs(o.U[i] - o.U_first[i]));
  for (int b = 0; b < B; ++b)
    printf("%s candidate %2d: J %.6f iterations %d; da %.4f db %.4f entry %g capped %g; CR_STEP_RISK before the last round %.3g\n", name, b, o.J[b],
           o.iters[b], o.tg[4 * b], o.tg[4 * b + 1], o.tg[4 * b + 2], o.tg[4 * b + 3], o.risk_before[b]);
  printf("%s: pick by hand %d; the rounds moved U by up to %.3g\n", name, want, moved);
  if (want < 0 || !(moved > 1e-3) || !(o.tg[0] > 0.1)) { printf("%s: the scene does not exercise the tightening\n", name); return false; }

  iLQR planner(sc.params, 0, M, B);
  planner.set_global_plan(sc.path);
  planner.set_Obstacle(sc.obstacles);
  planner.set_candidate_pick(pick, 0.0);
  if (with_cov) planner.set_obstacle_covariance(std::vector<double>(kCov, kCov + 3));
  if (with_check) planner.set_pose_covariance_check(sc.sigma0, sc.W, kMaxRisk);
  planner.set_chance_tightening(sc.sigma0, sc.W, kEps, rounds, kCap);
  const int best = planner.run_candidates(sc.egos);
  if (best != want) { printf("%s: run_candidates picked %d, the sequence by hand %d\n", name, best, want); return false; }
  if (!results_match(name, planner, o, B, best)) return false;
  if (with_check ? planner.last_chance_risk.size() != crisk.size() || !same(planner.last_chance_risk.data(), crisk.data(), crisk.size()) ||
                       !same(planner.last_step_risk.data(), cstep.data(), cstep.size())
                 : !planner.last_chance_risk.empty()) {
    printf("%s: last_chance_risk differs from cilqr_chance_risk on the final plans against the original obstacle\n", name);
    return false;
  }
  if (scored ? planner.last_scores.size() != score.size() || !same(planner.last_scores.data(), score.data(), score.size()) : !planner.last_scores.empty()) {
    printf("%s: last_scores differs from cilqr_score_batch on the final plans against the original obstacle\n", name);
    return false;
  }
  if (with_check || scored || rounds != 1 || with_cov) return true;
  // 4. the off switches: the plain pick on the first solve, nothing of the tightening left
  for (int off = 0; off < 2; ++off) {
    iLQR plain(sc.params, 0, M, B);
    plain.set_global_plan(sc.path);
    plain.set_Obstacle(sc.obstacles);
    plain.set_chance_tightening(sc.sigma0, sc.W, kEps, 1, kCap);
    if (off) plain.set_chance_tightening(nullptr, nullptr, kEps); else plain.set_chance_tightening(sc.sigma0, sc.W, kEps, 0);
    const int pick0 = plain.run_candidates(sc.egos);
    if (pick0 < 0 || !plain.last_tighten.empty() || !plain.last_tighten_risk_before.empty() ||
        !same(plain.U_result.a.data(), &o.U_first[(size_t)pick0 * 2 * N], 2 * (size_t)N)) {
      printf("%s: the tightening is not off\n", off ? "Sigma0 == nullptr" : "rounds == 0");
      return false;
    }
  }
  return true;
}

// The stored-rows pose-noise check (set_pose_noise_check, not fused) behind one round of tightening: the rollouts start from the final
// plans and are scored against the ORIGINAL obstacle.
bool stored_rows_case(const Scene& sc, int B) {
  const int S = 32;
  const double max_risk = 0.1;
  const std::vector<double> offsets = make_offsets(S);
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, B * S, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }  // (holds the B*S rows)
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), Xr((size_t)B * S * 4 * (N + 1)), Ur((size_t)B * S * 2 * N);
  std::vector<double> rows((size_t)B * S * CILQR_SCORE_FIELDS), risk((size_t)B * CILQR_RISK_FIELDS), total(B);
  std::vector<int32_t> ok(B);
  Hand o;
  const cilqr_obstacles obs{kPose, kDim, nullptr, 0, 1, 0, 0};
  const bool done =
      cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      by_hand(h, sc, B, sc.egos.data(), poly.data(), fl.data(), 1, false, o) &&
      cilqr_gains_batch(h, B, N, M, o.X.data(), o.U.data(), poly.data(), fl.data(), &obs, 1.0, o.k.data(), o.K.data(), ok.data()) == CILQR_OK &&
      cilqr_rollout_batch(h, B, N, S, o.X.data(), o.U.data(), o.k.data(), o.K.data(), offsets.data(), 0, 0.0, Xr.data(), Ur.data()) == CILQR_OK &&
      cilqr_score_rollouts(h, B, N, M, S, Xr.data(), Ur.data(), poly.data(), fl.data(), &obs, max_risk, rows.data(), risk.data(), total.data()) == CILQR_OK;
  if (!done) { printf("stored rows: the sequence by hand failed: %s\n", cilqr_last_error()); return false; }
  cilqr_destroy(h);
  const int want = first_minimum(total);
  double moved = 0.0;
  for (size_t i = 0; i < o.U.size(); ++i) moved = std::fmax(moved, std::fabs(o.U[i] - o.U_first[i]));
  printf("stored rows: pick by hand %d; %d of %d candidates rejected; the round moved U by up to %.3g\n", want, count_nan(total), B, moved);
  if (want < 0 || !(moved > 1e-3) || !(o.tg[0] > 0.1)) { printf("stored rows: the scene does not exercise the tightening\n"); return false; }
  iLQR planner(sc.params, 0, M, B);
  planner.set_global_plan(sc.path);
  planner.set_Obstacle(sc.obstacles);
  planner.set_pose_noise_check(offsets, max_risk);
  planner.set_chance_tightening(sc.sigma0, sc.W, kEps, 1, kCap);
  const int best = planner.run_candidates(sc.egos);
  if (best != want) { printf("stored rows: run_candidates picked %d, the sequence by hand %d\n", best, want); return false; }
  if (!results_match("stored rows", planner, o, B, best)) return false;
  if (!same(planner.last_risk, risk)) { printf("stored rows: last_risk differs from cilqr_score_rollouts on the final plans against the original obstacle\n"); return false; }
  if (!planner.last_scores.empty() || !planner.last_step_hits.empty() || !planner.last_chance_risk.empty()) {
    printf("stored rows: a field the mode does not produce is not empty\n");
    return false;
  }
  return true;
}

bool run_step_case(const Scene& sc) {
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, 3, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  const double* ego = &sc.egos[4 * 5];  // the candidate that starts 0.5 m beside the path
  double poly[CILQR_POLY_COEFFS], fl[2];
  std::vector<double> ref(2 * (size_t)sc.params.num_of_local_wpts);
  int n = 0;
  Hand o;
  bool done = cilqr_local_plan(&sc.params, sc.path.a.data(), sc.path.cols, ego, poly, ref.data(), &n) == CILQR_OK && n > 0;
  if (done) { fl[0] = ref[0]; fl[1] = ref[2 * (size_t)(n - 1)]; }
  done = done && by_hand(h, sc, 1, ego, poly, fl, 2, true, o);
  cilqr_destroy(h);
  if (!done) return false;
  iLQR planner(sc.params, 0, M, 1);
  planner.set_global_plan(sc.path);
  planner.set_Obstacle(sc.obstacles);
  planner.set_obstacle_covariance(std::vector<double>(kCov, kCov + 3));
  planner.set_chance_tightening(sc.sigma0, sc.W, kEps, 2, kCap);
  planner.run_step(ego);
  printf("run_step: J %.6f iterations %d; da %.4f db %.4f; CR_STEP_RISK before the last round %.3g\n", planner.last_cost, planner.last_iterations,
         planner.last_tighten.empty() ? -1.0 : planner.last_tighten[0], planner.last_tighten.empty() ? -1.0 : planner.last_tighten[1],
         planner.last_tighten_risk_before.empty() ? -1.0 : planner.last_tighten_risk_before[0]);
  if (!results_match("run_step", planner, o, 1, 0)) return false;
  // the warm start persists: a second tick starts from the tightened plan's U
  planner.set_chance_tightening(nullptr, nullptr, kEps);
  planner.clear_Obstacle();
  planner.run_step(ego);
  return planner.last_tighten.empty();
}

}  // namespace

int main() {
  Scene sc;
  sc.params = default_parameters();
  sc.params.horizon = N;
  const int B = 16;
  sc.path = straight_path();
  sc.egos = spread_egos(B, -3.0, 0.5);
  sc.obstacles = {standing_obstacle(sc.params, N, kPose[0], kPose[1], kPose[3], kDim[0], kDim[1])};
  sc.sigma0[0] = 0.16 * 0.16; sc.sigma0[5] = 0.16 * 0.16; sc.sigma0[15] = 0.017 * 0.017;
  sc.W[0] = 1e-4; sc.W[5] = 1e-4; sc.W[10] = 4e-4; sc.W[15] = 1e-6;

  if (!run_case(sc, "J", B, CandidatePick::MinTrackingCost, 1, false, false)) return 1;
  if (!run_case(sc, "total", B, CandidatePick::MinTotalCost, 1, false, false)) return 1;
  if (!run_case(sc, "two rounds, obs_cov", B, CandidatePick::MinTrackingCost, 2, true, false)) return 1;
  printf("tightened pick ok\n");
  printf("off switches ok\n");
  if (!run_case(sc, "check J", B, CandidatePick::MinTrackingCost, 1, false, true)) return 1;
  if (!run_case(sc, "check total", B, CandidatePick::MinTotalCost, 2, true, true)) return 1;
  if (!stored_rows_case(sc, B)) return 1;
  printf("composed pick ok\n");
  if (!run_step_case(sc)) return 1;
  printf("run_step ok\n");

  // 5. the conflict, in both orders
  const std::vector<double> samples(3 * 2, 0.05);
  {
    iLQR p(sc.params, 0, 4, B);
    p.set_chance_tightening(sc.sigma0, nullptr, kEps);
    if (!throws_logic_error([&] { p.set_obstacle_samples(samples, 2); }, "set_chance_tightening")) {
      printf("set_obstacle_samples after set_chance_tightening did not throw std::logic_error naming the conflict\n");
      return 1;
    }
    p.set_chance_tightening(sc.sigma0, nullptr, kEps, 0);  // (off: no conflict)
    p.set_obstacle_samples(samples, 2);
    if (!throws_logic_error([&] { p.set_chance_tightening(sc.sigma0, nullptr, kEps); }, "set_obstacle_samples")) {
      printf("set_chance_tightening after set_obstacle_samples did not throw\n");
      return 1;
    }
    p.set_chance_tightening(nullptr, nullptr, kEps);  // (off: no conflict)
  }
  printf("conflicts throw ok\n");
  return 0;
}
