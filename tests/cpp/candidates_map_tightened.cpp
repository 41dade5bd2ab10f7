// candidates_map_tightened.cpp — iLQR::run_candidates and run_step under map tightening (set_map_tightening): candidates side by side on
// a straight path, NO obstacle, and an uncertainty map with one blob beside the path — the configuration of the live node, where the map
// is all the planner knows of obstacles.  Pose noise as a covariance, Sigma0 = diag(0.16^2, 0.16^2, 0, 0.017^2), and a small process noise.
//   1. with the tightening set, run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_solve_batch with the map
//      set, then `rounds` times cilqr_gains_batch(lamb 1), cilqr_chance_risk (M = 0, sigma_out), cilqr_tighten_map(kappa of eps,
//      max_inflate) on the ORIGINAL map, and, candidate by candidate, its tightened layer set and cilqr_solve_batch from the U before (a
//      solve's bits do not depend on the batch it sits in), then the original map set again; the pick: strict-< first minimum of J, or
//      under MinTotalCost of cilqr_score_batch's total against the ORIGINAL map — with X_result / U_result / last_cost / last_iterations
//      / last_exit of that candidate, last_tighten_map and last_tighten_map_risk_before (0: no obstacle) equal to that sequence's, bit
//      for bit; one round and two;
//   2. the map on the handle: cilqr_debug_uncertainty_cost through iLQR::debug_map_cost gives the same bits before the setter, with it on,
//      and after the rounds; and last_scores (computed behind the rounds) is cilqr_score_batch's against the original map;
//   3. run_step: the same sequence at B = 1 behind cilqr_local_plan;
//   4. rounds = 0 and Sigma0 == nullptr switch it off: every output of run_candidates equals a planner's that never heard of it;
//   5. together with set_obstacle_samples, whichever comes second throws std::logic_error; together with a set_chance_tightening that
//      disagrees on Sigma0, W, lamb or rounds, the second setter throws std::logic_error; one that agrees composes: with obstacles set
//      one round tightens both and re-solves once; with the map tightening on (with W), set_chance_tightening switched off either way
//      leaves the map tightening's inputs alone: run_candidates equals the map-only run bit for bit.
// argv[1], if given: a dump of the first case for the restated pipeline of tests/test_tighten_map.py.
// Prints "map tightened pick ok", "map restored ok", "run_step ok", "off switches ok", "conflicts throw ok", "chance off beside map ok" and "composed ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 25, B = 6;
const double kEps = 0.05, kCap = 1.0;
const double kGeom[5] = {16.0, 8.0, 0.1, 6.0, 0.0}, kMapPose[3] = {0.0, 0.0, 0.05};
const double kBlob[3] = {6.0, -1.4, 0.7};  // world x, y of the blob's centre and its width
const double kPose[4] = {9.0, 2.6, 0.0, 0.0}, kDim[2] = {4.79, 2.16};  // the obstacle of the composed case: ahead, to the other side


struct Scene {
  Parameters params;
  Matrix path{2, 200};
  std::vector<double> egos;
  Uncertainty map;
  double sigma0[16] = {}, W[16] = {};
};

// The sequence by hand for nb solves whose path fit is given; everything it leaves.
struct Hand {
  std::vector<double> U, X, J, U_first, X_first, tm, risk_before, K, k, sigma;
  std::vector<float> layers;
  std::vector<int32_t> iters, status;
};

bool by_hand(cilqr_handle* h, const Scene& sc, int nb, const double* egos, const double* poly, const double* fl, int rounds, Hand& o) {
  const size_t cells = sc.map.layer.size();
  o.U = default_controls(nb, N); o.X.assign((size_t)nb * 4 * (N + 1), 0.0); o.J.assign(nb, 0.0);
  o.iters.assign(nb, 0); o.status.assign(nb, 0);
  o.k.assign((size_t)nb * 2 * N, 0.0); o.K.assign((size_t)nb * 8 * N, 0.0);
  o.tm.assign((size_t)nb * CILQR_TIGHTEN_MAP_FIELDS, 0.0); o.risk_before.assign(nb, 0.0);
  o.sigma.assign((size_t)nb * (N + 1) * 16, 0.0); o.layers.assign((size_t)nb * cells, 0.0f);
  std::vector<double> risk((size_t)nb * CILQR_CHANCE_FIELDS);
  std::vector<int32_t> ok(nb);
  const cilqr_uncertainty_map original = abi_map(sc.map, sc.map.layer.data());
  const double kappa = cilqr_chance_kappa(kEps);
  bool done = cilqr_set_uncertainty_map(h, &original) == CILQR_OK &&
              cilqr_solve_batch(h, nb, N, 0, egos, o.U.data(), poly, fl, nullptr, nullptr, nullptr, o.X.data(), o.J.data(), o.iters.data(),
                                o.status.data(), CILQR_FLAG_NONE) == CILQR_OK;
  o.U_first = o.U;
  o.X_first = o.X;
  for (int r = 0; r < rounds && done; ++r) {
    done = cilqr_gains_batch(h, nb, N, 0, o.X.data(), o.U.data(), poly, fl, nullptr, 1.0, o.k.data(), o.K.data(), ok.data()) == CILQR_OK &&
           cilqr_chance_risk(h, nb, N, 0, o.X.data(), o.U.data(), o.K.data(), sc.sigma0, 0, sc.W, nullptr, 0u, 1.0, nullptr, risk.data(), nullptr,
                             nullptr, o.sigma.data(), nullptr) == CILQR_OK &&
           cilqr_tighten_map(h, nb, N, o.X.data(), o.sigma.data(), kappa, kCap, o.layers.data(), o.tm.data()) == CILQR_OK;
    for (int b = 0; b < nb && done; ++b) {  // the host form of the map takes one shared layer: candidate by candidate
      const cilqr_uncertainty_map tight = abi_map(sc.map, &o.layers[(size_t)b * cells]);
      done = cilqr_set_uncertainty_map(h, &tight) == CILQR_OK &&
             cilqr_solve_batch(h, 1, N, 0, egos + 4 * b, &o.U[(size_t)b * 2 * N], poly + CILQR_POLY_COEFFS * b, fl + 2 * b, nullptr, nullptr, nullptr,
                               &o.X[(size_t)b * 4 * (N + 1)], &o.J[b], &o.iters[b], &o.status[b], CILQR_FLAG_NONE) == CILQR_OK;
    }
    done = done && cilqr_set_uncertainty_map(h, &original) == CILQR_OK;
    for (int b = 0; b < nb; ++b) o.risk_before[b] = risk[(size_t)b * CILQR_CHANCE_FIELDS + CILQR_CR_STEP_RISK];
  }
  if (!done) printf("the sequence by hand failed: %s\n", cilqr_last_error());
  return done;
}

bool results_match(const char* name, const iLQR& p, const Hand& o, int nb, int best) {
  if (p.last_tighten_map.size() != o.tm.size() || !same(p.last_tighten_map.data(), o.tm.data(), o.tm.size()) ||
      p.last_tighten_map_risk_before.size() != (size_t)nb || !same(p.last_tighten_map_risk_before.data(), o.risk_before.data(), nb)) {
    printf("%s: last_tighten_map / last_tighten_map_risk_before differ from the sequence by hand\n", name);
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

bool map_cost(const iLQR& p, const std::vector<double>& states, std::vector<double>& out) {
  try {
    out = p.debug_map_cost(states);
  } catch (const std::exception& e) {
    printf("debug_map_cost: %s\n", e.what());
    return false;
  }
  return true;
}

void dump(const char* path, const Scene& sc, const Hand& o, const std::vector<double>& poly, const std::vector<double>& fl, int best) {
  FILE* f = fopen(path, "w");
  if (!f) return;
  const auto put = [f](const double* v, size_t n) { for (size_t i = 0; i < n; ++i) fprintf(f, "%.17g\n", v[i]); };
  fprintf(f, "%d %d %d %d %d\n", B, N, sc.map.geom.rows, sc.map.geom.cols, best);
  const double head[3] = {cilqr_chance_kappa(kEps), kCap, sc.params.w_uncertainty};
  put(head, 3); put(kGeom, 5); put(kMapPose, 3);
  put(sc.egos.data(), sc.egos.size()); put(poly.data(), poly.size()); put(fl.data(), fl.size());
  put(o.X_first.data(), o.X_first.size()); put(o.U_first.data(), o.U_first.size()); put(o.K.data(), o.K.size());
  put(sc.sigma0, 16); put(sc.W, 16);
  put(o.X.data(), o.X.size()); put(o.U.data(), o.U.size()); put(o.J.data(), o.J.size()); put(o.tm.data(), o.tm.size());
  for (int32_t v : o.iters) fprintf(f, "%d\n", v);
  for (float v : sc.map.layer) fprintf(f, "%.9g\n", (double)v);
  for (float v : o.layers) fprintf(f, "%.9g\n", (double)v);
  fclose(f);
}

// One configuration of run_candidates: by hand on a handle of its own, then a fresh planner.
bool run_case(const Scene& sc, const char* name, CandidatePick pick, int rounds, const char* dump_path) {
  cilqr_handle* h = nullptr;
  // (the host form of cilqr_tighten_map stages its layers through the arena: B*(20*N + 26 + cells/2) doubles against
  // max_batch*(22*N + 34); a solve's bits do not depend on the handle's max_batch)
  if (cilqr_create(&sc.params, 16 * B, N, 0, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2);
  Hand o;
  const bool scored = pick == CandidatePick::MinTotalCost;
  std::vector<double> score((size_t)B * CILQR_SCORE_FIELDS), total(B);
  bool done = cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
              by_hand(h, sc, B, sc.egos.data(), poly.data(), fl.data(), rounds, o);
  // what follows judges the final plan against the ORIGINAL map (by_hand left it on the handle)
  if (done && scored) done = cilqr_score_batch(h, B, N, 0, o.X.data(), o.U.data(), poly.data(), fl.data(), nullptr, 0.0, score.data(), total.data()) == CILQR_OK;
  if (!done) { printf("%s: the sequence by hand failed: %s\n", name, cilqr_last_error()); return false; }
  cilqr_destroy(h);
  const int want = first_minimum(scored ? total : o.J);
  double moved = 0.0;
  for (size_t i = 0; i < o.U.size(); ++i) moved = std::fmax(moved, std::fabs(o.U[i] - o.U_first[i]));
  for (int b = 0; b < B; ++b)
    printf("%s candidate %d: J %.6f iterations %d; raised %g max raise %.4g at cell %g reach %.4f capped %g lost %g\n", name, b, o.J[b], o.iters[b],
           o.tm[6 * b], o.tm[6 * b + 1], o.tm[6 * b + 2], o.tm[6 * b + 3], o.tm[6 * b + 4], o.tm[6 * b + 5]);
  printf("%s: pick by hand %d; the rounds moved U by up to %.3g\n", name, want, moved);
  if (want < 0 || !(moved > 1e-3) || !(o.tm[0] > 100.0)) { printf("%s: the scene does not exercise the tightening\n", name); return false; }
  if (dump_path) dump(dump_path, sc, o, poly, fl, want);

  std::vector<double> states((size_t)4 * B * N), cost0, cost1, cost2;  // the first plans' states: where the map matters
  for (int b = 0; b < B; ++b) memcpy(&states[(size_t)4 * b * N], &o.X_first[(size_t)b * 4 * (N + 1)], 4 * (size_t)N * sizeof(double));
  iLQR planner(sc.params, 0, 0, B);
  planner.set_global_plan(sc.path);
  planner.set_uncertainty_map(sc.map);
  planner.set_candidate_pick(pick, 0.0);
  if (!map_cost(planner, states, cost0)) return false;
  planner.set_map_tightening(sc.sigma0, sc.W, kEps, rounds, kCap);
  if (!map_cost(planner, states, cost1)) return false;
  const int best = planner.run_candidates(sc.egos);
  if (!map_cost(planner, states, cost2)) return false;
  if (best != want) { printf("%s: run_candidates picked %d, the sequence by hand %d\n", name, best, want); return false; }
  if (!results_match(name, planner, o, B, best)) return false;
  double largest = 0.0;
  for (int i = 0; i < B * N; ++i) largest = std::fmax(largest, cost0[i]);
  if (!(largest > 0.1) || !same(cost0.data(), cost1.data(), cost0.size()) || !same(cost0.data(), cost2.data(), cost0.size())) {
    printf("%s: the map on the handle is not the original one, bit for bit (largest cost %.3g)\n", name, largest);
    return false;
  }
  if (scored ? planner.last_scores.size() != score.size() || !same(planner.last_scores.data(), score.data(), score.size()) : !planner.last_scores.empty()) {
    printf("%s: last_scores differs from cilqr_score_batch on the final plans against the original map\n", name);
    return false;
  }
  if (!planner.last_tighten.empty() || !planner.last_tighten_risk_before.empty()) { printf("%s: last_tighten is filled without obstacles\n", name); return false; }
  // a second tick: the warm start is the pick's U, the map still the original
  const int again = planner.run_candidates(sc.egos);
  if (again < 0 || planner.last_tighten_map.size() != (size_t)B * CILQR_TIGHTEN_MAP_FIELDS) { printf("%s: the second tick failed\n", name); return false; }
  if (scored || rounds != 1) return true;
  // 4. the off switches: every output equals a planner's that never heard of the setter
  iLQR never(sc.params, 0, 0, B);
  never.set_global_plan(sc.path);
  never.set_uncertainty_map(sc.map);
  const int pick_never = never.run_candidates(sc.egos);
  for (int off = 0; off < 2; ++off) {
    iLQR plain(sc.params, 0, 0, B);
    plain.set_global_plan(sc.path);
    plain.set_map_tightening(sc.sigma0, sc.W, kEps, 1, kCap);
    plain.set_uncertainty_map(sc.map);
    if (off) plain.set_map_tightening(nullptr, nullptr, kEps); else plain.set_map_tightening(sc.sigma0, sc.W, kEps, 0);
    const int pick0 = plain.run_candidates(sc.egos);
    if (pick0 != pick_never || pick0 < 0 || !plain.last_tighten_map.empty() || !plain.last_tighten_map_risk_before.empty() ||
        !same(plain.U_result.a.data(), never.U_result.a.data(), 2 * (size_t)N) || !same(plain.X_result.a.data(), never.X_result.a.data(), 4 * (size_t)(N + 1)) ||
        !same(&plain.last_cost, &never.last_cost, 1) || plain.last_iterations != never.last_iterations || plain.last_exit != never.last_exit ||
        !same(plain.U_result.a.data(), &o.U_first[(size_t)pick0 * 2 * N], 2 * (size_t)N)) {
      printf("%s: the map tightening is not off\n", off ? "Sigma0 == nullptr" : "rounds == 0");
      return false;
    }
  }
  return true;
}

bool run_step_case(const Scene& sc) {
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, 16, N, 0, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  const double* ego = &sc.egos[0];  // the candidate that passes closest to the blob
  double poly[CILQR_POLY_COEFFS], fl[2];
  std::vector<double> ref(2 * (size_t)sc.params.num_of_local_wpts);
  int n = 0;
  Hand o;
  bool done = cilqr_local_plan(&sc.params, sc.path.a.data(), sc.path.cols, ego, poly, ref.data(), &n) == CILQR_OK && n > 0;
  if (done) { fl[0] = ref[0]; fl[1] = ref[2 * (size_t)(n - 1)]; }
  done = done && by_hand(h, sc, 1, ego, poly, fl, 2, o);
  cilqr_destroy(h);
  if (!done) return false;
  iLQR planner(sc.params, 0, 0, 1);
  planner.set_global_plan(sc.path);
  planner.set_uncertainty_map(sc.map);
  planner.set_map_tightening(sc.sigma0, sc.W, kEps, 2, kCap);
  planner.run_step(ego);
  printf("run_step: J %.6f iterations %d; raised %g reach %.4f\n", planner.last_cost, planner.last_iterations,
         planner.last_tighten_map.empty() ? -1.0 : planner.last_tighten_map[0], planner.last_tighten_map.empty() ? -1.0 : planner.last_tighten_map[3]);
  if (!results_match("run_step", planner, o, 1, 0)) return false;
  // with the map cleared the rounds are skipped and nothing of them is left
  planner.clear_uncertainty_map();
  planner.run_step(ego);
  return planner.last_tighten_map.empty() && planner.last_tighten_map_risk_before.empty();
}

// 5c. both tightenings, with an obstacle set: one round = gains -> chance risk (M = 1) -> both tighten calls -> ONE re-solve on the
// inflated obstacle and the tightened layer.
bool composed_case(const Scene& sc) {
  const int M = 1;
  const double* ego = &sc.egos[0];
  cilqr_handle* h = nullptr;
  if (cilqr_create(&sc.params, 16, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  const size_t cells = sc.map.layer.size();
  double poly[CILQR_POLY_COEFFS], fl[2], J = 0.0, tg[CILQR_TIGHTEN_FIELDS], tm[CILQR_TIGHTEN_MAP_FIELDS], risk[CILQR_CHANCE_FIELDS];
  std::vector<double> ref(2 * (size_t)sc.params.num_of_local_wpts), U(2 * (size_t)N), X(4 * (size_t)(N + 1)), k(2 * (size_t)N), K(8 * (size_t)N);
  std::vector<double> sigma((size_t)(N + 1) * 16), tpose((size_t)4 * N), tdim((size_t)2 * N);
  std::vector<float> layer(cells);
  int32_t iters = 0, status = 0, ok = 0;
  int n = 0;
  const cilqr_obstacles obs{kPose, kDim, nullptr, 0, 1, 0, 0};
  const cilqr_obstacles inflated{tpose.data(), tdim.data(), nullptr, (int64_t)M * N, N, 1, 0};
  const cilqr_uncertainty_map original = abi_map(sc.map, sc.map.layer.data()), tight = abi_map(sc.map, layer.data());
  const double kappa = cilqr_chance_kappa(kEps);
  cilqr_default_control_seq(N, U.data());
  bool done = cilqr_local_plan(&sc.params, sc.path.a.data(), sc.path.cols, ego, poly, ref.data(), &n) == CILQR_OK && n > 0;
  if (done) { fl[0] = ref[0]; fl[1] = ref[2 * (size_t)(n - 1)]; }
  done = done && cilqr_set_uncertainty_map(h, &original) == CILQR_OK &&
         cilqr_solve_batch_obstacles(h, 1, N, M, ego, U.data(), poly, fl, &obs, X.data(), &J, &iters, &status, CILQR_FLAG_NONE) == CILQR_OK &&
         cilqr_gains_batch(h, 1, N, M, X.data(), U.data(), poly, fl, &obs, 1.0, k.data(), K.data(), &ok) == CILQR_OK &&
         cilqr_chance_risk(h, 1, N, M, X.data(), U.data(), K.data(), sc.sigma0, 0, sc.W, &obs, 0u, 1.0, nullptr, risk, nullptr, nullptr, sigma.data(),
                           nullptr) == CILQR_OK &&
         cilqr_tighten_obstacles(h, 1, N, M, X.data(), sigma.data(), &obs, nullptr, kappa, 2.0, tpose.data(), tdim.data(), tg) == CILQR_OK &&
         cilqr_tighten_map(h, 1, N, X.data(), sigma.data(), kappa, kCap, layer.data(), tm) == CILQR_OK &&
         cilqr_set_uncertainty_map(h, &tight) == CILQR_OK &&
         cilqr_solve_batch_obstacles(h, 1, N, M, ego, U.data(), poly, fl, &inflated, X.data(), &J, &iters, &status, CILQR_FLAG_NONE) == CILQR_OK;
  if (!done) printf("composed: the sequence by hand failed: %s\n", cilqr_last_error());
  cilqr_destroy(h);
  if (!done) return false;
  iLQR planner(sc.params, 0, M, 1);
  planner.set_global_plan(sc.path);
  planner.set_Obstacle({standing_obstacle(sc.params, N, kPose[0], kPose[1], kPose[3], kDim[0], kDim[1])});
  planner.set_uncertainty_map(sc.map);
  planner.set_chance_tightening(sc.sigma0, sc.W, kEps, 1, 2.0);
  planner.set_map_tightening(sc.sigma0, sc.W, kEps, 1, kCap);
  planner.run_step(ego);
  printf("composed: J %.6f iterations %d; da %.4f; raised %g; CR_STEP_RISK before %.3g\n", planner.last_cost, planner.last_iterations,
         planner.last_tighten.empty() ? -1.0 : planner.last_tighten[0], planner.last_tighten_map.empty() ? -1.0 : planner.last_tighten_map[0], risk[0]);
  return planner.last_tighten.size() == CILQR_TIGHTEN_FIELDS && same(planner.last_tighten.data(), tg, CILQR_TIGHTEN_FIELDS) &&
         planner.last_tighten_map.size() == CILQR_TIGHTEN_MAP_FIELDS && same(planner.last_tighten_map.data(), tm, CILQR_TIGHTEN_MAP_FIELDS) &&
         planner.last_tighten_risk_before.size() == 1 && same(planner.last_tighten_risk_before.data(), &risk[CILQR_CR_STEP_RISK], 1) &&
         same(planner.last_tighten_map_risk_before.data(), &risk[CILQR_CR_STEP_RISK], 1) && same(planner.X_result.a.data(), X.data(), X.size()) &&
         same(planner.U_result.a.data(), U.data(), U.size()) && same(&planner.last_cost, &J, 1) && planner.last_iterations == iters;
}

}  // namespace

int main(int argc, char** argv) {
  Scene sc;
  sc.params = default_parameters();
  sc.params.horizon = N;
  sc.params.safe_length = 1.1; sc.params.safe_width = 0.9;
  sc.params.w_uncertainty = 5.0;  // (at the default 1 the map term is too weak to move a plan off the blob)
  sc.path = straight_path();
  sc.egos = spread_egos(B, -1.0, 0.4, 4.0);
  if (cilqr_map_geom_set(&sc.map.geom, kGeom[0], kGeom[1], kGeom[2], kGeom[3], kGeom[4]) != CILQR_OK) return 1;
  sc.map.pose_x = kMapPose[0]; sc.map.pose_y = kMapPose[1]; sc.map.pose_theta = kMapPose[2];
  const cilqr_map_geom& g = sc.map.geom;
  sc.map.layer.resize((size_t)g.rows * g.cols);
  const double x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res);
  const double c = std::cos(kMapPose[2]), s = std::sin(kMapPose[2]);
  for (int j = 0; j < g.cols; ++j)
    for (int i = 0; i < g.rows; ++i) {
      const double mx = x_first - i * g.res, my = y_first - j * g.res;
      const double wx = kMapPose[0] + c * mx - s * my, wy = kMapPose[1] + s * mx + c * my;
      const double r2 = (wx - kBlob[0]) * (wx - kBlob[0]) + (wy - kBlob[1]) * (wy - kBlob[1]);
      sc.map.layer[(size_t)j * g.rows + i] = (float)(100.0 * std::tanh(1.3 * std::exp(-0.5 * r2 / (kBlob[2] * kBlob[2]))));
    }
  sc.sigma0[0] = 0.16 * 0.16; sc.sigma0[5] = 0.16 * 0.16; sc.sigma0[15] = 0.017 * 0.017;
  sc.W[0] = 1e-4; sc.W[5] = 1e-4; sc.W[10] = 4e-4; sc.W[15] = 1e-6;

  if (!run_case(sc, "J", CandidatePick::MinTrackingCost, 1, argc > 1 ? argv[1] : nullptr)) return 1;
  printf("off switches ok\n");
  if (!run_case(sc, "total", CandidatePick::MinTotalCost, 1, nullptr)) return 1;
  if (!run_case(sc, "two rounds", CandidatePick::MinTotalCost, 2, nullptr)) return 1;
  printf("map tightened pick ok\n");
  printf("map restored ok\n");
  if (!run_step_case(sc)) return 1;
  printf("run_step ok\n");

  // 5. the conflicts
  const std::vector<double> samples(3 * 2, 0.05);
  {
    iLQR p(sc.params, 0, 4, B);
    p.set_map_tightening(sc.sigma0, nullptr, kEps);
    if (!throws_logic_error([&] { p.set_obstacle_samples(samples, 2); }, "set_map_tightening")) {
      printf("set_obstacle_samples after set_map_tightening did not throw std::logic_error naming the conflict\n");
      return 1;
    }
    p.set_map_tightening(sc.sigma0, nullptr, kEps, 0);  // (off: no conflict)
    p.set_obstacle_samples(samples, 2);
    if (!throws_logic_error([&] { p.set_map_tightening(sc.sigma0, nullptr, kEps); }, "set_obstacle_samples")) {
      printf("set_map_tightening after set_obstacle_samples did not throw\n");
      return 1;
    }
    p.set_obstacle_samples({}, 0);
    double other[16];
    memcpy(other, sc.sigma0, sizeof(other));
    other[0] *= 2.0;
    p.set_chance_tightening(sc.sigma0, sc.W, kEps);
    if (!throws_logic_error([&] { p.set_map_tightening(other, sc.W, kEps); }, "must agree") ||
        !throws_logic_error([&] { p.set_map_tightening(sc.sigma0, nullptr, kEps); }, "must agree") ||
        !throws_logic_error([&] { p.set_map_tightening(sc.sigma0, sc.W, kEps, 1, kCap, 2.0); }, "must agree") ||
        !throws_logic_error([&] { p.set_map_tightening(sc.sigma0, sc.W, kEps, 2); }, "must agree")) {
      printf("a set_map_tightening that disagrees with set_chance_tightening did not throw\n");
      return 1;
    }
    p.set_map_tightening(sc.sigma0, sc.W, kEps);  // (agrees: composes)
    if (!throws_logic_error([&] { p.set_chance_tightening(other, sc.W, kEps); }, "must agree")) {
      printf("a set_chance_tightening that disagrees with set_map_tightening did not throw\n");
      return 1;
    }
  }
  printf("conflicts throw ok\n");
  // 5b. the chance tightening switched off beside a map tightening that has W: both off switches, with a null W and with another W
  {
    iLQR only(sc.params, 0, 0, B);
    only.set_global_plan(sc.path);
    only.set_uncertainty_map(sc.map);
    only.set_map_tightening(sc.sigma0, sc.W, kEps, 1, kCap);
    const int want = only.run_candidates(sc.egos);
    double other_W[16];
    memcpy(other_W, sc.W, sizeof(other_W));
    other_W[0] *= 100.0;
    for (int off = 0; off < 3; ++off) {
      iLQR p(sc.params, 0, 0, B);
      p.set_global_plan(sc.path);
      p.set_uncertainty_map(sc.map);
      if (off == 2) p.set_chance_tightening(sc.sigma0, sc.W, kEps, 1);  // (on first, in agreement, then off)
      p.set_map_tightening(sc.sigma0, sc.W, kEps, 1, kCap);
      if (off == 0) p.set_chance_tightening(nullptr, nullptr, kEps);
      else p.set_chance_tightening(sc.sigma0, other_W, kEps, 0);
      const int best = p.run_candidates(sc.egos);
      if (want < 0 || best != want || p.last_tighten_map.size() != only.last_tighten_map.size() ||
          !same(p.last_tighten_map.data(), only.last_tighten_map.data(), only.last_tighten_map.size()) ||
          !same(p.X_result.a.data(), only.X_result.a.data(), only.X_result.a.size()) ||
          !same(p.U_result.a.data(), only.U_result.a.data(), only.U_result.a.size()) || !same(&p.last_cost, &only.last_cost, 1) ||
          p.last_iterations != only.last_iterations || !p.last_tighten.empty()) {
        printf("set_chance_tightening switched off (%d) beside a map tightening changed the map-only run\n", off);
        return 1;
      }
    }
  }
  printf("chance off beside map ok\n");
  if (!composed_case(sc)) { printf("composed: run_step differs from the sequence by hand\n"); return 1; }
  printf("composed ok\n");
  return 0;
}
