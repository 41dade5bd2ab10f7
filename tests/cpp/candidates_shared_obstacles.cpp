// candidates_shared_obstacles.cpp — iLQR::run_candidates, which hands its one obstacle set to every candidate by strides
// (cilqr_solve_batch_obstacles, batch stride 0; step stride 0 where every column is the same), against what it replaced: the
// set replicated B times into the dense [B][M][N] tables of cilqr_solve_batch, followed by the strict-< first-minimum pick.
// Static and moving obstacles, from a fresh planner each (the same default warm start).  Prints "bit-identical" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 50, M = 4, B = 96;
  Parameters params = default_parameters();
  params.horizon = N;
  Matrix path(2, 200);
  for (int i = 0; i < 200; ++i) { path(0, i) = 1.0 * i; path(1, i) = 1.5 * std::sin(0.05 * i + 0.3); }
  std::vector<double> egos(4 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    egos[4 * b + 0] = 20.0 + 0.3 * std::sin(1.7 * b);
    egos[4 * b + 1] = 1.5 * std::sin(1.3) + 0.3 * std::cos(2.3 * b);
    egos[4 * b + 2] = 4.0 + 0.2 * std::sin(0.7 * b);
    egos[4 * b + 3] = 0.05 + 0.03 * std::cos(1.1 * b);
  }
  for (int moving = 0; moving < 2; ++moving) {
    std::vector<Obstacle> obstacles;
    for (int o = 0; o < M; ++o) {
      Matrix dim(2, N), pose(4, N);
      const double v = moving ? 1.0 + 0.5 * o : 0.0, th = 0.1 * o - 0.15;
      for (int t = 0; t < N; ++t) {
        dim(0, t) = 4.79; dim(1, t) = 2.16;
        pose(0, t) = 28.0 + 9.0 * o + v * std::cos(th) * 0.1 * t;
        pose(1, t) = ((o % 2) ? -1.8 : 2.2) + v * std::sin(th) * 0.1 * t;
        pose(2, t) = v; pose(3, t) = th;
      }
      obstacles.emplace_back(params, dim, pose);
    }
    iLQR planner(params, 0, M, B);
    planner.set_global_plan(path);
    planner.set_Obstacle(obstacles);
    const int best = planner.run_candidates(egos);

    // by hand: the same pre-step, B copies of the obstacle set, the dense solve, the pick
    cilqr_handle* h = nullptr;
    if (cilqr_create(&params, B, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
    std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
    std::vector<int32_t> iters(B), status(B);
    if (cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) != CILQR_OK) {
      printf("cilqr_local_plan_batch: %s\n", cilqr_last_error());
      return 1;
    }
    std::vector<double> pose((size_t)B * M * 4 * N), dim((size_t)B * M * 2 * N);
    for (int b = 0; b < B; ++b)
      for (int m = 0; m < M; ++m)
        for (int t = 0; t < N; ++t) {
          for (int r = 0; r < 4; ++r) pose[(((size_t)b * M + m) * N + t) * 4 + r] = obstacles[m].relative_pos_array(r, t);
          for (int r = 0; r < 2; ++r) dim[(((size_t)b * M + m) * N + t) * 2 + r] = obstacles[m].dimension(r, t);
        }
    if (cilqr_solve_batch(h, B, N, M, egos.data(), U.data(), poly.data(), fl.data(), pose.data(), dim.data(), nullptr, X.data(), J.data(),
                          iters.data(), status.data(), CILQR_FLAG_NONE) != CILQR_OK) {
      printf("cilqr_solve_batch: %s\n", cilqr_last_error());
      return 1;
    }
    cilqr_destroy(h);
    int want = 0;
    bool have = false;
    for (int b = 0; b < B; ++b)
      if (J[b] == J[b] && (!have || J[b] < J[want])) { want = b; have = true; }
    const char* kind = moving ? "moving" : "static";
    if (best != want) { printf("%s: run_candidates picked %d, the dense pick is %d\n", kind, best, want); return 1; }
    if (!same(planner.X_result.a.data(), &X[(size_t)want * 4 * (N + 1)], 4 * (size_t)(N + 1)) ||
        !same(planner.U_result.a.data(), &U[(size_t)want * 2 * N], 2 * (size_t)N) || !same(&planner.last_cost, &J[want], 1) ||
        planner.last_iterations != iters[want] || planner.last_exit != status[want]) {
      printf("%s: the picked candidate's X / U / J / iterations / exit differ from the dense solve\n", kind);
      return 1;
    }
    printf("%s obstacles: candidate %d of %d, J = %.17g\n", kind, best, B, J[want]);
  }
  printf("bit-identical\n");
  return 0;
}
