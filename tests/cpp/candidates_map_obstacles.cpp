// candidates_map_obstacles.cpp — iLQR::run_candidates under set_map_obstacles: the six candidates of candidates_map_clearance.cpp,
// x0 = (0, -1 + 0.4 b, 4, 0) beside a straight path, NO obstacle given, and an uncertainty map with one blob at (6, -1.4) — the
// configuration of the live node, where the occupied cells are all the planner knows of obstacles.  Seeds are the cells above
// kThreshold = 50; tests/test_map_obstacles.py asserts the scene's figures from the CPU oracle and the restatements.
//   1. by hand, on a handle whose arena holds the map: cilqr_map_distance -> cilqr_map_obstacles (one row: the blob's box) -> the
//      solve with that row as a static obstacle shared by the batch, and the solve without it;
//   2. under set_map_obstacles run_candidates gives the hand-written solve's pick, X, U and cost bit for bit, and last_map_obstacles
//      and last_map_obstacle_counts are the rows and n_out of the hand-written call;
//   3. the rows stand behind the obstacles of set_Obstacle, survive set_Obstacle and clear_Obstacle, and go with clear_uncertainty_map
//      and with on = false;
//   4. with the setter off — never called, or called and switched off — every result is the solve without the row, bit for bit;
//   5. with set_tracked_obstacles, set_obstacle_samples or set_obstacle_covariance in force a run throws std::logic_error; rows beyond
//      max_obstacles and bad arguments throw std::runtime_error.
// Prints "rows: ...", "J: ..." and "map obstacles ok" on success.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 25, B = 6, K = 4, kMinCells = 3;
  const double kThreshold = 50.0, inf = INFINITY;
  const double kGeom[5] = {16.0, 8.0, 0.1, 6.0, 0.0}, kMapPose[3] = {0.0, 0.0, 0.05}, kBlob[3] = {6.0, -1.4, 0.7};
  Parameters params = default_parameters();
  params.horizon = N;
  params.safe_length = 1.1; params.safe_width = 0.9;
  params.w_uncertainty = 5.0;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, -1.0, 0.4, 4.0);
  Uncertainty map;
  if (cilqr_map_geom_set(&map.geom, kGeom[0], kGeom[1], kGeom[2], kGeom[3], kGeom[4]) != CILQR_OK) return 1;
  map.pose_x = kMapPose[0]; map.pose_y = kMapPose[1]; map.pose_theta = kMapPose[2];
  const cilqr_map_geom& g = map.geom;
  const size_t cells = (size_t)g.rows * g.cols;
  map.layer.resize(cells);
  const double x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res);
  const double c = std::cos(kMapPose[2]), s = std::sin(kMapPose[2]);
  for (int j = 0; j < g.cols; ++j)
    for (int i = 0; i < g.rows; ++i) {
      const double mx = x_first - i * g.res, my = y_first - j * g.res;
      const double wx = kMapPose[0] + c * mx - s * my, wy = kMapPose[1] + s * mx + c * my;
      const double r2 = (wx - kBlob[0]) * (wx - kBlob[0]) + (wy - kBlob[1]) * (wy - kBlob[1]);
      map.layer[(size_t)j * g.rows + i] = (float)(100.0 * std::tanh(1.3 * std::exp(-0.5 * r2 / (kBlob[2] * kBlob[2]))));
    }

  // 1. by hand (max_batch 64: the arena then holds the map's three arrays)
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, 64, N, K, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<int32_t> d2(cells), work(cells), label(cells), n_out(4);
  std::vector<double> comp((size_t)K * CILQR_MAP_OBSTACLE_FIELDS), boxes((size_t)K * 5), pose_out((size_t)K * 4), dim_out((size_t)K * 2);
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<double> U0 = default_controls(B, N), X0(X.size()), J0(B);
  std::vector<int32_t> iters(B), status(B), iters0(B), status0(B);
  const cilqr_uncertainty_map original = abi_map(map);
  if (cilqr_set_uncertainty_map(h, &original) != CILQR_OK ||
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) != CILQR_OK ||
      cilqr_map_distance(h, 1, map.layer.data(), 0, &g, kThreshold, 0u, d2.data(), nullptr) != CILQR_OK ||
      cilqr_map_obstacles(h, 1, d2.data(), &g, 0, 0u, kMapPose, 0, K, kMinCells, inf, 0.0, work.data(), label.data(), n_out.data(), comp.data(),
                          boxes.data(), pose_out.data(), dim_out.data()) != CILQR_OK) {
    printf("by hand: %s\n", cilqr_last_error());
    return 1;
  }
  const int rows = n_out[2];
  if (rows != 1 || n_out[0] != 1) { printf("by hand: %d rows of %d components, the scene has one blob\n", rows, n_out[0]); return 1; }
  const cilqr_obstacles obs = {pose_out.data(), dim_out.data(), nullptr, 0, 1, 0, 0};
  if (cilqr_solve_batch_obstacles(h, B, N, rows, egos.data(), U.data(), poly.data(), fl.data(), &obs, X.data(), J.data(), iters.data(), status.data(),
                                  CILQR_FLAG_NONE) != CILQR_OK ||
      cilqr_solve_batch(h, B, N, 0, egos.data(), U0.data(), poly.data(), fl.data(), nullptr, nullptr, nullptr, X0.data(), J0.data(), iters0.data(),
                        status0.data(), CILQR_FLAG_NONE) != CILQR_OK) {
    printf("by hand: %s\n", cilqr_last_error());
    return 1;
  }
  cilqr_destroy(h);
  printf("rows:");
  for (int k = 0; k < 5 * rows; ++k) printf(" %.9f", boxes[k]);
  printf("\nJ:");
  for (int b = 0; b < B; ++b) printf(" %.9f", J[b]);
  printf("\nJ0:");
  for (int b = 0; b < B; ++b) printf(" %.9f", J0[b]);
  printf("\n");
  if (same(X, X0)) { printf("by hand: the row changes no plan\n"); return 1; }
  const std::vector<double> want_rows(boxes.begin(), boxes.begin() + 5 * rows);

  const auto matches = [&](iLQR& q, int best, const std::vector<double>& Xw, const std::vector<double>& Uw, const std::vector<double>& Jw,
                           const std::vector<int32_t>& itw) {
    return best == first_minimum(Jw) && same(q.X_result.a.data(), &Xw[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1)) &&
           same(q.U_result.a.data(), &Uw[(size_t)best * 2 * N], 2 * (size_t)N) && q.last_cost == Jw[best] && q.last_iterations == itw[best];
  };
  // 2. the setter in front of the map, and behind it
  for (int order = 0; order < 2; ++order) {
    iLQR q(params, 0, K, B);
    q.set_global_plan(path);
    if (order == 0) q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K);
    q.set_uncertainty_map(map);
    if (order == 1) q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K);
    if (!same(q.last_map_obstacles, want_rows) || memcmp(q.last_map_obstacle_counts, n_out.data(), 4 * sizeof(int32_t)) != 0) {
      printf("order %d: last_map_obstacles differs from the rows of cilqr_map_obstacles\n", order);
      return 1;
    }
    const int best = q.run_candidates(egos);
    if (!matches(q, best, X, U, J, iters)) { printf("order %d: run_candidates differs from the hand-written sequence (picked %d)\n", order, best); return 1; }
  }
  // 3. behind set_Obstacle's obstacles; kept over set_Obstacle and clear_Obstacle; removed with the map and with on = false
  {
    iLQR q(params, 0, K, B);
    q.set_global_plan(path);
    q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K);
    q.set_uncertainty_map(map);
    q.set_Obstacle({standing_obstacle(params, N, 40.0, 30.0)});  // (far away: present, and felt by nobody's pick)
    int best = q.run_candidates(egos);
    if (best < 0 || !same(q.last_map_obstacles, want_rows)) { printf("behind set_Obstacle: the rows are gone\n"); return 1; }
    q.clear_Obstacle();
    best = q.run_candidates(egos);
    if (best < 0 || !same(q.last_map_obstacles, want_rows)) { printf("after clear_Obstacle: the rows are gone\n"); return 1; }
    q.clear_uncertainty_map();
    if (!q.last_map_obstacles.empty() || q.last_map_obstacle_counts[2] != 0) { printf("clear_uncertainty_map left the rows\n"); return 1; }
    q.set_uncertainty_map(map);
    if (!same(q.last_map_obstacles, want_rows)) { printf("the map set again: no rows\n"); return 1; }
    q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K, false);
    if (!q.last_map_obstacles.empty()) { printf("on = false left the rows\n"); return 1; }
  }
  // 4. off: the solve without the row
  for (int touched = 0; touched < 2; ++touched) {
    iLQR q(params, 0, K, B);
    q.set_global_plan(path);
    if (touched) {
      q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K);
      q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K, false);
    }
    q.set_uncertainty_map(map);
    const int best = q.run_candidates(egos);
    if (!matches(q, best, X0, U0, J0, iters0) || !q.last_map_obstacles.empty()) { printf("off (%d): the run is not the solve without the row\n", touched); return 1; }
  }
  // 5. what the setter does not define, and its limits
  {
    iLQR q(params, 0, K, B);
    q.set_global_plan(path);
    q.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K);
    q.set_uncertainty_map(map);
    q.set_obstacle_covariance({0.1, 0.0, 0.1});
    if (!throws_logic_error([&] { (void)q.run_candidates(egos); }, "set_map_obstacles")) { printf("a covariance beside the rows was accepted\n"); return 1; }
    q.set_obstacle_covariance({});
    q.set_tracked_obstacles({20.0, 5.0, 1.0, 0.0, 0.0, 0.0}, {4.0, 2.0}, {}, {});
    if (!throws_logic_error([&] { (void)q.run_candidates(egos); }, "set_map_obstacles")) { printf("tracks beside the rows were accepted\n"); return 1; }
    iLQR tight(params, 0, 1, B);  // one obstacle allowed: the far one and the blob's row are two
    tight.set_global_plan(path);
    tight.set_Obstacle({standing_obstacle(params, N, 40.0, 30.0)});
    tight.set_map_obstacles(kThreshold, 0.0, kMinCells, inf, 0.0, K);
    bool refused = false;
    try { tight.set_uncertainty_map(map); } catch (const std::runtime_error&) { refused = true; }
    if (!refused) { printf("rows beyond max_obstacles were accepted\n"); return 1; }
    for (int bad = 0; bad < 5; ++bad) {
      refused = false;
      try {
        q.set_map_obstacles(bad == 0 ? NAN : kThreshold, bad == 1 ? -0.1 : 0.0, bad == 2 ? 0 : kMinCells, bad == 3 ? 0.0 : inf, 0.0, bad == 4 ? 1025 : K);
      } catch (const std::runtime_error&) { refused = true; }
      if (!refused) { printf("bad argument %d was accepted\n", bad); return 1; }
    }
  }
  printf("map obstacles ok\n");
  return 0;
}
