// candidates_risk_map.cpp — iLQR::run_candidates with the map risk check (set_map_risk_check) under the fused pose-noise check
// (set_pose_noise_check_fused) while an uncertainty map is set: the scene of candidates_risk_fused.cpp — one static obstacle 1 m
// beside a straight path, candidates spread laterally across it, 70 start offsets of the size of the node's pose noise — and a
// vehicle-frame costmap with a smooth, moderately occupied region (at most 66 of 100: cheap for the map cost, above the threshold
// of 50) just ahead of the candidates that start nearest to the path — the ones the obstacle check accepts and the cost prefers —
// and a few unknown (NaN) cells.
//   1. run_candidates returns the index the C-ABI sequence called by hand gives — cilqr_set_uncertainty_map,
//      cilqr_solve_batch_obstacles, cilqr_gains_batch(lamb 1), cilqr_score_batch (nominal totals), cilqr_rollout_risk(k_scale 0,
//      max_risk, base = those totals), cilqr_rollout_risk_map(k_scale 0, occ_threshold, map max_risk, base = that total), strict-<
//      first minimum of its `total` — with X_result / U_result / last_cost of that candidate, and last_map_risk,
//      last_map_step_hits, last_map_unknown_hits, last_risk and last_step_hits equal to that sequence's, bit for bit;
//   2. the map rejects candidates the obstacle check accepts, and the pick differs from the pick without the map check;
//   3. with unknown_hits the unknown rows hit too: no fewer rejections, and the fields are again the hand-called sequence's;
//   4. without a map (clear_uncertainty_map), and with the check switched off (a NaN threshold), run_candidates behaves as under
//      set_pose_noise_check_fused alone: last_map_* empty;
//   5. with every candidate rejected by the map (max_risk = -1) the call returns -1 and the results are untouched.
// With a file name as its argument it writes what a checker needs to derive the map risk and the pick on its own: the sizes
// (B, N, S, rows, cols), the threshold, the map max_risk, the pick, the map geometry and pose, then X, U, the gains k and K, the
// obstacle check's total (the base), the offsets, last_map_risk, last_map_step_hits, last_map_unknown_hits and the layer, as text,
// one value per line.
// Prints "map risk pick ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main(int argc, char** argv) {
  const int N = 30, M = 1, B = 16, S = 70;
  const double max_risk = 0.1, threshold = 50.0, map_max_risk = 0.1;
  const int RR = CILQR_ROLLOUT_RISK_FIELDS, MR = CILQR_MAP_RISK_FIELDS;
  Parameters params = default_parameters();
  params.horizon = N;
  params.safe_length = 1.1;  // the launch file's values (Experiment.launch:7-8)
  params.safe_width = 0.9;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, -3.0, 0.5);
  const std::vector<Obstacle> obstacles{standing_obstacle(params, N, 12.0, -1.0)};
  const std::vector<double> offsets = make_offsets(S);

  // the costmap: 200 x 80 cells of 0.2 m centred 15 m ahead; cell (i, j) has its centre at (34.9 - 0.2 i, 7.9 - 0.2 j); a smooth
  // occupied region around (3.5, -0.6) and a weaker one around (20, -4.5); six unknown cells near the candidates' starts
  Uncertainty um;
  if (!bump_costmap(um, {{80.0, 3.5, -0.6, 1.5, 0.5}, {60.0, 20.0, -4.5, 5.0, 1.5}})) return 1;
  const int rows = um.geom.rows, cols = um.geom.cols;
  const int nan_cells[6][2] = {{170, 52}, {171, 52}, {168, 47}, {165, 38}, {166, 38}, {150, 26}};
  for (const auto& c : nan_cells) um.layer[(size_t)c[1] * rows + c[0]] = NAN;

  // by hand: the host-buffer forms
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  const cilqr_uncertainty_map m = abi_map(um);
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B), ok(B);
  const double pose1[4] = {12.0, -1.0, 0.0, 0.0}, dim1[2] = {4.79, 2.16};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};  // one set for the batch, constant over the horizon
  std::vector<double> k((size_t)B * 2 * N), K((size_t)B * 8 * N), score((size_t)B * CILQR_SCORE_FIELDS), base(B), risk((size_t)B * RR), total(B);
  std::vector<int32_t> hits((size_t)B * N);
  std::vector<double> mrisk((size_t)B * MR), mtotal(B), urisk((size_t)B * MR), utotal(B), ntotal(B);
  std::vector<int32_t> mhits((size_t)B * N), munk((size_t)B * N), uhits((size_t)B * N), uunk((size_t)B * N);
  const bool done =
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_set_uncertainty_map(h, &m) == CILQR_OK &&
      cilqr_solve_batch_obstacles(h, B, N, M, egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(),
                                  status.data(), CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_gains_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), ok.data()) == CILQR_OK &&
      cilqr_score_batch(h, B, N, M, X.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, score.data(), base.data()) == CILQR_OK &&
      cilqr_rollout_risk(h, B, N, M, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, &obs, max_risk, base.data(),
                         risk.data(), hits.data(), total.data()) == CILQR_OK &&
      cilqr_rollout_risk_map(h, B, N, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, threshold, 0u, map_max_risk,
                             total.data(), mrisk.data(), mhits.data(), munk.data(), mtotal.data()) == CILQR_OK &&
      cilqr_rollout_risk_map(h, B, N, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, threshold,
                             CILQR_MAP_RISK_UNKNOWN_HITS, map_max_risk, total.data(), urisk.data(), uhits.data(), uunk.data(),
                             utotal.data()) == CILQR_OK &&
      cilqr_rollout_risk_map(h, B, N, S, X.data(), U.data(), k.data(), K.data(), offsets.data(), 0, 0.0, threshold, 0u, -1.0, total.data(),
                             mrisk.data(), nullptr, nullptr, ntotal.data()) == CILQR_OK;
  if (!done) { printf("the sequence by hand failed: %s\n", cilqr_last_error()); return 1; }
  cilqr_destroy(h);
  const int want = first_minimum(mtotal), want_obstacles_only = first_minimum(total), want_unknown = first_minimum(utotal);
  for (int b = 0; b < B; ++b) {
    const double *r = &risk[(size_t)RR * b], *q = &mrisk[(size_t)MR * b];
    printf("candidate %2d: nominal total %.6f obstacle risk %.4f | map risk %.4f worst occupancy %.4f (row %g, entry %g) first step %g "
           "step share %.4f unknown %.4f (with unknown hits: %.4f)\n",
           b, base[b], r[CILQR_RR_COLLISION], q[CILQR_MR_COLLISION], q[CILQR_MR_WORST_OCC], q[CILQR_MR_WORST_ROW], q[CILQR_MR_WORST_ENTRY],
           q[CILQR_MR_FIRST_STEP], q[CILQR_MR_STEP_SHARE], q[CILQR_MR_UNKNOWN], urisk[(size_t)MR * b + CILQR_MR_COLLISION]);
  }
  printf("pick by hand: %d (obstacles alone: %d, unknown hits: %d); rejected %d by the obstacles, %d with the map, %d with unknown hits\n",
         want, want_obstacles_only, want_unknown, count_nan(total), count_nan(mtotal), count_nan(utotal));
  // 2. the scene separates the checks
  if (want < 0 || want == want_obstacles_only || count_nan(mtotal) <= count_nan(total) || count_nan(mtotal) == B ||
      count_nan(utotal) < count_nan(mtotal) || first_minimum(ntotal) != -1) {
    printf("the scene does not separate the candidates by map risk\n");
    return 1;
  }
  bool any_unknown = false;
  for (int b = 0; b < B; ++b) any_unknown = any_unknown || (mrisk[(size_t)MR * b + CILQR_MR_UNKNOWN] > 0.0 && mrisk[(size_t)MR * b + CILQR_MR_UNKNOWN] < 1.0);
  if (!any_unknown) { printf("no candidate has an unknown share strictly between 0 and 1\n"); return 1; }

  iLQR planner(params, 0, M, B);
  planner.set_global_plan(path);
  planner.set_Obstacle(obstacles);
  planner.set_uncertainty_map(um);
  planner.set_pose_noise_check_fused(offsets, max_risk);
  // 1. the check set
  planner.set_map_risk_check(threshold, map_max_risk);
  const int best = planner.run_candidates(egos);
  if (best != want) { printf("the check picked %d, the sequence by hand %d\n", best, want); return 1; }
  if (planner.last_map_risk.size() != mrisk.size() || !same(planner.last_map_risk.data(), mrisk.data(), mrisk.size()) ||
      !same_i(planner.last_map_step_hits, mhits) || !same_i(planner.last_map_unknown_hits, munk)) {
    printf("last_map_risk / last_map_step_hits / last_map_unknown_hits differ from cilqr_rollout_risk_map on the same solves\n");
    return 1;
  }
  if (planner.last_risk.size() != risk.size() || !same(planner.last_risk.data(), risk.data(), risk.size()) || !same_i(planner.last_step_hits, hits) ||
      planner.last_scores.size() != score.size() || !same(planner.last_scores.data(), score.data(), score.size())) {
    printf("last_risk / last_step_hits / last_scores differ from the hand-called sequence\n");
    return 1;
  }
  if (!same(planner.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
      !same(planner.U_result.a.data(), &U[(size_t)best * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[best], 1) ||
      planner.last_iterations != iters[best] || planner.last_exit != status[best]) {
    printf("the pick's X / U / J differ from the hand-written solve\n");
    return 1;
  }
  if (argc > 1) {
    FILE* f = fopen(argv[1], "w");
    if (!f) { printf("cannot write %s\n", argv[1]); return 1; }
    fprintf(f, "%d\n%d\n%d\n%d\n%d\n%.17g\n%.17g\n%d\n", B, N, S, rows, cols, threshold, map_max_risk, best);
    for (double v : kBumpGeom) fprintf(f, "%.17g\n", v);
    for (double v : kBumpMapPose) fprintf(f, "%.17g\n", v);
    put(f, X); put(f, U); put(f, k); put(f, K); put(f, total); put(f, offsets); put(f, planner.last_map_risk);
    put_i(f, planner.last_map_step_hits); put_i(f, planner.last_map_unknown_hits);
    for (float v : um.layer) fprintf(f, "%.9g\n", (double)v);
    fclose(f);
  }
  // 5. every candidate rejected by the map: results stay
  const Matrix X_before = planner.X_result, U_before = planner.U_result;
  const double cost_before = planner.last_cost;
  planner.set_map_risk_check(threshold, -1.0);
  const int none = planner.run_candidates(egos);
  if (none != -1) { printf("every candidate rejected by the map, yet the pick is %d\n", none); return 1; }
  if (!same(planner.U_result.a.data(), U_before.a.data(), U_before.a.size()) ||
      !same(planner.X_result.a.data(), X_before.a.data(), X_before.a.size()) || !same(&planner.last_cost, &cost_before, 1) ||
      planner.last_map_risk.size() != mrisk.size()) {
    printf("all rejected: results were touched\n");
    return 1;
  }
  // 3. unknown rows hit too.  (The warm start is still the default one: the rejected call above left it alone, and a fresh planner
  // shows the same.)
  {
    iLQR fresh(params, 0, M, B);
    fresh.set_global_plan(path);
    fresh.set_Obstacle(obstacles);
    fresh.set_uncertainty_map(um);
    fresh.set_pose_noise_check_fused(offsets, max_risk);
    fresh.set_map_risk_check(threshold, map_max_risk, true);
    const int ub = fresh.run_candidates(egos);
    if (ub != want_unknown || fresh.last_map_risk.size() != urisk.size() || !same(fresh.last_map_risk.data(), urisk.data(), urisk.size()) ||
        !same_i(fresh.last_map_step_hits, uhits) || !same_i(fresh.last_map_unknown_hits, uunk)) {
      printf("unknown hits: pick %d, by hand %d, or the fields differ\n", ub, want_unknown);
      return 1;
    }
    // 4. the check switched off, then no map: the fused check alone.  (The warm start is the pick's U now, so only the modes are checked.)
    fresh.set_map_risk_check(NAN, map_max_risk);
    const int off = fresh.run_candidates(egos);
    if (off < 0 || !fresh.last_map_risk.empty() || !fresh.last_map_step_hits.empty() || !fresh.last_map_unknown_hits.empty() ||
        fresh.last_risk.size() != risk.size()) {
      printf("check off: pick %d, last_map_risk not empty\n", off);
      return 1;
    }
    fresh.set_map_risk_check(threshold, map_max_risk);
    fresh.clear_uncertainty_map();
    const int no_map = fresh.run_candidates(egos);
    if (no_map < 0 || !fresh.last_map_risk.empty() || fresh.last_risk.size() != risk.size()) {
      printf("no map: pick %d, last_map_risk not empty\n", no_map);
      return 1;
    }
  }
  // 4. without the map the obstacle-only pick comes back on a planner that starts from the default warm start
  {
    iLQR plain(params, 0, M, B);
    plain.set_global_plan(path);
    plain.set_Obstacle(obstacles);
    plain.set_uncertainty_map(um);
    plain.set_pose_noise_check_fused(offsets, max_risk);
    const int pb = plain.run_candidates(egos);
    if (pb != want_obstacles_only || !plain.last_map_risk.empty()) { printf("no map check: pick %d, by hand %d\n", pb, want_obstacles_only); return 1; }
  }
  printf("map risk pick ok\n");
  return 0;
}
