// candidates_chance_map.cpp — iLQR::run_candidates with the map covariance check (set_map_covariance_check) under the pose-covariance
// check (set_pose_covariance_check) while an uncertainty map is set: the scene and the costmap of candidates_risk_map.cpp — a straight
// path, candidates spread laterally across it, a smooth occupied region (at most 66 of 100, above the threshold of 50) just ahead of
// the candidates that start nearest to the path, a few unknown cells — with the node's pose noise given as a covariance,
// Sigma0 = diag(0.16^2, 0.16^2, 0, 0.017^2).
//   1. "live": no obstacle set, the live node's case — the chance call runs with M = 0 for its Sigma_t alone and rejects nothing.
//      run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_set_uncertainty_map,
//      cilqr_solve_batch_obstacles, cilqr_gains_batch(lamb 1), cilqr_chance_risk (sigma_out; base = J), cilqr_chance_risk_map on the
//      5 x 5 x 3 nodes of cilqr_pose_quadrature (base = that total), strict-< first minimum of its `total` — with X_result / U_result
//      / last_cost of that candidate and last_chance_map_risk, last_map_step_risk, last_chance_risk equal to that sequence's, bit for
//      bit.  The map rejects some candidates and not all, and the pick differs from the pick of the covariance check alone;
//   2. "obstacle": the same with the obstacle of candidates_chance.cpp set, under MinTotalCost, with sum_bound and unknown_hits, and
//      with set_map_risk_check composing behind it (chance -> map covariance -> map rollout on the zero offset);
//   3. without a map (clear_uncertainty_map), and with the check switched off (a NaN threshold), run_candidates behaves as under
//      set_pose_covariance_check alone — the pick is that check's — and last_chance_map_risk / last_map_step_risk are empty; so they
//      are without the covariance check;
//   4. with every candidate rejected by the map (max_risk = -1) the call returns -1 and the results are untouched.
// With a file name as its argument it writes what a checker needs to derive the "live" case's map risk and pick on its own: the sizes
// (B, N, Q, rows, cols), the threshold, max_risk, the pick, the map geometry and pose, then X, U, the gains K, the chance call's total
// (the base), Sigma0, the nodes, the weights, last_chance_map_risk, last_map_step_risk and the layer, as text, one value per line.
// Prints "map covariance pick ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 30, B = 16, NX = 5, NY = 5, NTH = 3, Q = NX * NY * NTH, CM = CILQR_CHANCE_MAP_FIELDS;
const double kThreshold = 50.0, kMapMaxRisk = 0.1, kChanceMaxRisk = 0.2, kRolloutMapMaxRisk = 0.5;


struct Scene {
  Parameters params;
  Matrix path{2, 200};
  std::vector<double> egos;
  std::vector<Obstacle> obstacles;
  Uncertainty um;
  double sigma0[16] = {};
};

struct ByHand {
  std::vector<double> X, U, J, K, total, cmrisk, cmstep, cmtotal, crisk, nodes, weights, final_total;
  std::vector<int32_t> iters, status;
};

// The C-ABI sequence on a handle of its own.  with_obstacle: M = 1 and MinTotalCost's nominal totals as the base, else M = 0 and J.
bool by_hand(const Scene& sc, bool with_obstacle, bool with_map, uint32_t flags, double map_max_risk, bool rollout_map, ByHand& o) {
  const int M = with_obstacle ? 1 : 0;
  cilqr_handle* h = nullptr;
  // (max_batch 2 B: the host form of cilqr_chance_risk with sigma_out fits the arena for B <= max_batch / 2)
  if (cilqr_create(&sc.params, 2 * B, N, 1, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  const cilqr_uncertainty_map m = abi_map(sc.um);
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), k((size_t)B * 2 * N), score((size_t)B * CILQR_SCORE_FIELDS), base(B);
  std::vector<double> sigma((size_t)B * (N + 1) * 16), mrisk((size_t)B * CILQR_MAP_RISK_FIELDS), mtotal(B);
  std::vector<int32_t> ok(B);
  o.X.assign((size_t)B * 4 * (N + 1), 0.0); o.J.assign(B, 0.0); o.K.assign((size_t)B * 8 * N, 0.0);
  o.total.assign(B, 0.0); o.cmrisk.assign((size_t)B * CM, 0.0); o.cmstep.assign((size_t)B * N, 0.0); o.cmtotal.assign(B, 0.0);
  o.crisk.assign((size_t)B * CILQR_CHANCE_FIELDS, 0.0); o.nodes.assign((size_t)Q * 3, 0.0); o.weights.assign(Q, 0.0);
  o.iters.assign(B, 0); o.status.assign(B, 0);
  o.U = default_controls(B, N);
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16}, zero[4] = {0.0, 0.0, 0.0, 0.0};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};
  const cilqr_obstacles* po = M ? &obs : nullptr;
  bool done = cilqr_pose_quadrature(NX, NY, NTH, o.nodes.data(), o.weights.data()) == CILQR_OK &&
              cilqr_local_plan_batch(h, B, sc.path.cols, sc.path.a.data(), 0, sc.egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
              (!with_map || cilqr_set_uncertainty_map(h, &m) == CILQR_OK) &&
              cilqr_solve_batch_obstacles(h, B, N, M, sc.egos.data(), o.U.data(), poly.data(), fl.data(), po, o.X.data(), o.J.data(),
                                          o.iters.data(), o.status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
              (!M || cilqr_score_batch(h, B, N, M, o.X.data(), o.U.data(), poly.data(), fl.data(), po, 1.0, score.data(), base.data()) == CILQR_OK) &&
              cilqr_gains_batch(h, B, N, M, o.X.data(), o.U.data(), poly.data(), fl.data(), po, 1.0, k.data(), o.K.data(), ok.data()) == CILQR_OK &&
              cilqr_chance_risk(h, B, N, M, o.X.data(), o.U.data(), o.K.data(), sc.sigma0, 0, nullptr, po, 0u, M ? kChanceMaxRisk : 1.0,
                                M ? base.data() : o.J.data(), o.crisk.data(), nullptr, nullptr, sigma.data(), o.total.data()) == CILQR_OK;
  o.final_total = o.total;
  if (done && with_map) {
    done = cilqr_chance_risk_map(h, B, N, Q, o.X.data(), sigma.data(), o.nodes.data(), o.weights.data(), kThreshold, flags, map_max_risk,
                                 o.total.data(), o.cmrisk.data(), o.cmstep.data(), nullptr, nullptr, o.cmtotal.data()) == CILQR_OK;
    o.final_total = o.cmtotal;
    if (done && rollout_map) {
      done = cilqr_rollout_risk_map(h, B, N, 1, o.X.data(), o.U.data(), k.data(), o.K.data(), zero, 0, 0.0, kThreshold, 0u, kRolloutMapMaxRisk,
                                    o.cmtotal.data(), mrisk.data(), nullptr, nullptr, mtotal.data()) == CILQR_OK;
      o.final_total = mtotal;
    }
  }
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return false; }
  cilqr_destroy(h);
  return true;
}

void configure(iLQR& p, const Scene& sc, bool with_obstacle, bool with_map) {
  p.set_global_plan(sc.path);
  if (with_obstacle) {
    p.set_Obstacle(sc.obstacles);
    p.set_candidate_pick(CandidatePick::MinTotalCost, 0.0);
  }
  if (with_map) p.set_uncertainty_map(sc.um);
  p.set_pose_covariance_check(sc.sigma0, nullptr, with_obstacle ? kChanceMaxRisk : 1.0);
}

bool results_are(const iLQR& p, const ByHand& o, int best) {
  return same(p.X_result.a.data(), &o.X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) &&
         same(p.U_result.a.data(), &o.U[(size_t)best * 2 * N], 2 * (size_t)N) && same(&p.last_cost, &o.J[best], 1) &&
         p.last_iterations == o.iters[best] && p.last_exit == o.status[best];
}
}  // namespace

int main(int argc, char** argv) {
  Scene sc;
  sc.params = default_parameters();
  sc.params.horizon = N;
  sc.params.safe_length = 1.1;  // the launch file's values (Experiment.launch:7-8)
  sc.params.safe_width = 0.9;
  sc.path = straight_path();
  sc.egos = spread_egos(B, -3.0, 0.5);
  sc.obstacles = {standing_obstacle(sc.params, N, 12.0, -1.0)};
  sc.sigma0[0] = 0.16 * 0.16; sc.sigma0[5] = 0.16 * 0.16; sc.sigma0[15] = 0.017 * 0.017;
  // the costmap of candidates_risk_map.cpp: 200 x 80 cells of 0.2 m centred 15 m ahead; cell (i, j) has its centre at
  // (34.9 - 0.2 i, 7.9 - 0.2 j); a smooth occupied region around (3.5, -0.6), a weaker one around (20, -4.5); six unknown cells
  if (!bump_costmap(sc.um, {{80.0, 3.5, -0.6, 1.5, 0.5}, {60.0, 20.0, -4.5, 5.0, 1.5}})) return 1;
  const int rows = sc.um.geom.rows, cols = sc.um.geom.cols;
  const int nan_cells[6][2] = {{170, 52}, {171, 52}, {168, 47}, {165, 38}, {166, 38}, {150, 26}};
  for (const auto& c : nan_cells) sc.um.layer[(size_t)c[1] * rows + c[0]] = NAN;

  // 1. the live node's case
  ByHand live, alone;
  if (!by_hand(sc, false, true, 0u, kMapMaxRisk, false, live) || !by_hand(sc, false, false, 0u, kMapMaxRisk, false, alone)) return 1;
  // (`alone`: the same scene solved with no map set, for the planners below that have none)
  const int want = first_minimum(live.cmtotal), want_chance = first_minimum(live.total), want_alone = first_minimum(alone.total);
  for (int b = 0; b < B; ++b) {
    const double* q = &live.cmrisk[(size_t)CM * b];
    printf("live candidate %2d: J %.6f | step risk %.6f (step %g) sum risk %.6f first step %g mean occ %.4f (step %g) worst occ %.4f unknown %.6f%s\n",
           b, live.J[b], q[CILQR_CM_STEP_RISK], q[CILQR_CM_WORST_STEP], q[CILQR_CM_SUM_RISK], q[CILQR_CM_FIRST_STEP], q[CILQR_CM_MEAN_OCC],
           q[CILQR_CM_MEAN_OCC_STEP], q[CILQR_CM_WORST_OCC], q[CILQR_CM_UNKNOWN], live.cmtotal[b] != live.cmtotal[b] ? "  rejected" : "");
  }
  printf("live: pick by hand %d (covariance check alone: %d); %d of %d rejected by the map\n", want, want_chance, count_nan(live.cmtotal), B);
  if (want < 0 || want == want_chance || count_nan(live.total) != 0 || count_nan(live.cmtotal) == 0 || count_nan(live.cmtotal) == B) {
    printf("the scene does not separate the candidates by map risk\n");
    return 1;
  }
  iLQR planner(sc.params, 0, 1, B);
  configure(planner, sc, false, true);
  planner.set_map_covariance_check(kThreshold, kMapMaxRisk);
  const int best = planner.run_candidates(sc.egos);
  if (best != want) { printf("live: the check picked %d, the sequence by hand %d\n", best, want); return 1; }
  if (!same(planner.last_chance_map_risk, live.cmrisk) || !same(planner.last_map_step_risk, live.cmstep) ||
      !same(planner.last_chance_risk, live.crisk)) {
    printf("live: last_chance_map_risk / last_map_step_risk / last_chance_risk differ from the hand-called sequence\n");
    return 1;
  }
  if (!results_are(planner, live, best)) { printf("live: the pick's X / U / J differ from the hand-written solve\n"); return 1; }
  if (argc > 1) {
    FILE* f = fopen(argv[1], "w");
    if (!f) { printf("cannot write %s\n", argv[1]); return 1; }
    fprintf(f, "%d\n%d\n%d\n%d\n%d\n%.17g\n%.17g\n%d\n", B, N, Q, rows, cols, kThreshold, kMapMaxRisk, best);
    for (double v : kBumpGeom) fprintf(f, "%.17g\n", v);
    for (double v : kBumpMapPose) fprintf(f, "%.17g\n", v);
    put(f, live.X); put(f, live.U); put(f, live.K); put(f, live.total);
    for (double v : sc.sigma0) fprintf(f, "%.17g\n", v);
    put(f, live.nodes); put(f, live.weights); put(f, planner.last_chance_map_risk); put(f, planner.last_map_step_risk);
    for (float v : sc.um.layer) fprintf(f, "%.9g\n", (double)v);
    fclose(f);
  }
  // 4. every candidate rejected by the map: results stay
  {
    const Matrix X_before = planner.X_result, U_before = planner.U_result;
    const double cost_before = planner.last_cost;
    planner.set_map_covariance_check(kThreshold, -1.0);
    const int none = planner.run_candidates(sc.egos);
    if (none != -1) { printf("every candidate rejected by the map, yet the pick is %d\n", none); return 1; }
    if (!same(planner.U_result.a.data(), U_before.a.data(), U_before.a.size()) ||
        !same(planner.X_result.a.data(), X_before.a.data(), X_before.a.size()) || !same(&planner.last_cost, &cost_before, 1) ||
        planner.last_chance_map_risk.size() != live.cmrisk.size()) {
      printf("all rejected: results were touched\n");
      return 1;
    }
  }
  // 3. no map, the check switched off, no covariance check: the covariance check alone (or nothing), and empty fields
  {
    iLQR p(sc.params, 0, 1, B);
    configure(p, sc, false, false);  // no map
    p.set_map_covariance_check(kThreshold, kMapMaxRisk);
    const int nb = p.run_candidates(sc.egos);
    if (nb != want_alone || !p.last_chance_map_risk.empty() || !p.last_map_step_risk.empty() || !same(p.last_chance_risk, alone.crisk) ||
        !results_are(p, alone, nb)) {
      printf("no map: pick %d, the covariance check alone by hand %d, or fields not empty\n", nb, want_alone);
      return 1;
    }
  }
  {
    iLQR p(sc.params, 0, 1, B);
    configure(p, sc, false, true);
    p.set_map_covariance_check(kThreshold, kMapMaxRisk);
    p.set_map_covariance_check(NAN, kMapMaxRisk);  // off
    const int ob = p.run_candidates(sc.egos);
    if (ob != want_chance || !p.last_chance_map_risk.empty() || !p.last_map_step_risk.empty() || !same(p.last_chance_risk, live.crisk)) {
      printf("check off: pick %d, by hand %d\n", ob, want_chance);
      return 1;
    }
    p.set_map_covariance_check(kThreshold, kMapMaxRisk);
    p.clear_uncertainty_map();
    if (p.run_candidates(sc.egos) < 0 || !p.last_chance_map_risk.empty()) { printf("map cleared: last_chance_map_risk not empty\n"); return 1; }
  }
  {
    iLQR p(sc.params, 0, 1, B);
    p.set_global_plan(sc.path);
    p.set_uncertainty_map(sc.um);
    p.set_map_covariance_check(kThreshold, kMapMaxRisk);  // no covariance check: nothing happens
    if (p.run_candidates(sc.egos) < 0 || !p.last_chance_map_risk.empty() || !p.last_map_step_risk.empty() || !p.last_chance_risk.empty()) {
      printf("no covariance check: the map covariance check did something\n");
      return 1;
    }
  }
  // 2. with an obstacle, MinTotalCost, sum_bound and unknown_hits; then the map rollout check behind it
  for (int chain = 0; chain < 2; ++chain) {
    ByHand o;
    const uint32_t flags = CILQR_CHANCE_MAP_BOUND_SUM | CILQR_CHANCE_MAP_UNKNOWN_HITS;
    if (!by_hand(sc, true, true, flags, kMapMaxRisk, chain == 1, o)) return 1;
    const int w = first_minimum(o.final_total);
    printf("obstacle%s: pick by hand %d; rejected %d by the chance value, %d with the map covariance, %d in the end\n", chain ? " + map rollout" : "", w,
           count_nan(o.total), count_nan(o.cmtotal), count_nan(o.final_total));
    if (count_nan(o.total) == 0 || count_nan(o.cmtotal) <= count_nan(o.total)) { printf("obstacle: the scene does not separate the checks\n"); return 1; }
    iLQR p(sc.params, 0, 1, B);
    configure(p, sc, true, true);
    p.set_map_covariance_check(kThreshold, kMapMaxRisk, NX, NY, NTH, true, true);
    if (chain) p.set_map_risk_check(kThreshold, kRolloutMapMaxRisk);
    const int ob = p.run_candidates(sc.egos);
    if (ob != w || !same(p.last_chance_map_risk, o.cmrisk) || !same(p.last_map_step_risk, o.cmstep) || !same(p.last_chance_risk, o.crisk) ||
        (chain ? p.last_map_risk.empty() : !p.last_map_risk.empty()) || (ob >= 0 && !results_are(p, o, ob))) {
      printf("obstacle%s: pick %d, by hand %d, or the fields differ\n", chain ? " + map rollout" : "", ob, w);
      return 1;
    }
  }
  printf("map covariance pick ok\n");
  return 0;
}
