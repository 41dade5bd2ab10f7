// candidates_path_frame.cpp — iLQR::set_path_frame: run_candidates and run_step in a frame along each candidate's slice of the path.
// The scene is the facade programs' own — a straight path along +x, candidates spread sideways, one standing obstacle beside the
// path — and the same scene turned by a quarter turn about the origin and moved by (3, 0): the road then heads north along x = 3.
//   1. setter off on the east road: the pick, X_result, U_result and last_cost are what a planner that never heard of the setter
//      returns, bit for bit, and last_frames stays empty (also after the setter was on and switched off again);
//   2. setter on, east road: the pick is the unframed one, X and U within 1e-9 (the frames are pure translations);
//   3. setter on, north road: the same pick, U within 1e-9 of the east road's, X_result and ref_traj_result the east road's turned
//      (1e-9): x_north = 3 - y_east, y_north = x_east, heading + pi/2; last_frames holds phi = pi/2 and last_frame_info 0;
//      without the setter the north road's plan is a different one (the unframed fit is a constant there);
//   4. the same through MinTotalCost (the score runs on the framed rows) and through run_step;
//   5. an in-block mode (the footprint check) together with the setter throws std::logic_error naming set_path_frame.
// Prints "path frame ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const double kHalfPi = 1.5707963267948966;

double max_abs_diff(const double* a, const double* b, size_t n) {
  double d = 0.0;
  for (size_t i = 0; i < n; ++i) d = std::fmax(d, std::fabs(a[i] - b[i]));
  return d;
}
// how far X_north is from X_east turned by a quarter turn and moved by (3, 0)
double turned_diff(const Matrix& Xn, const Matrix& Xe) {
  double d = 0.0;
  for (int t = 0; t < Xe.cols; ++t) {
    d = std::fmax(d, std::fabs(Xn(0, t) - (3.0 - Xe(1, t))));
    d = std::fmax(d, std::fabs(Xn(1, t) - Xe(0, t)));
    if (Xe.rows == 4) {
      d = std::fmax(d, std::fabs(Xn(2, t) - Xe(2, t)));
      d = std::fmax(d, std::fabs(Xn(3, t) - (Xe(3, t) + kHalfPi)));
    }
  }
  return d;
}
}  // namespace

int main() {
  const int N = 30, M = 1, B = 8;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix east = straight_path();
  Matrix north(2, east.cols);
  for (int i = 0; i < east.cols; ++i) { north(0, i) = 3.0 - east(1, i); north(1, i) = east(0, i); }
  const std::vector<double> egos_e = spread_egos(B, -1.4, 0.4);
  std::vector<double> egos_n(egos_e.size());
  for (int b = 0; b < B; ++b) {
    egos_n[4 * b + 0] = 3.0 - egos_e[4 * b + 1];
    egos_n[4 * b + 1] = egos_e[4 * b + 0];
    egos_n[4 * b + 2] = egos_e[4 * b + 2];
    egos_n[4 * b + 3] = egos_e[4 * b + 3] + kHalfPi;
  }
  const std::vector<Obstacle> obs_e{standing_obstacle(params, N, 12.0, -1.0, 0.1)};
  const std::vector<Obstacle> obs_n{standing_obstacle(params, N, 3.0 + 1.0, 12.0, 0.1 + kHalfPi)};

  // the planner as it is without the setter
  iLQR plain(params, 0, M, B);
  plain.set_global_plan(east);
  plain.set_Obstacle(obs_e);
  const int want = plain.run_candidates(egos_e);
  const Matrix Xe = plain.X_result, Ue = plain.U_result, Re = plain.ref_traj_result;
  const double Je = plain.last_cost;

  // 1. setter off (after having been on)
  {
    iLQR p(params, 0, M, B);
    p.set_global_plan(east);
    p.set_Obstacle(obs_e);
    p.set_path_frame(true);
    p.set_path_frame(false);
    const int best = p.run_candidates(egos_e);
    if (best != want || !same(p.X_result.a.data(), Xe.a.data(), Xe.a.size()) || !same(p.U_result.a.data(), Ue.a.data(), Ue.a.size()) ||
        !same(&p.last_cost, &Je, 1) || !same(p.ref_traj_result.a.data(), Re.a.data(), Re.a.size()) || !p.last_frames.empty()) {
      printf("setter off: the results differ from a planner without the setter\n");
      return 1;
    }
  }
  // 2. and 3.
  Matrix Un;
  {
    iLQR p(params, 0, M, B);
    p.set_global_plan(east);
    p.set_Obstacle(obs_e);
    p.set_path_frame(true);
    const int best = p.run_candidates(egos_e);
    const double dX = max_abs_diff(p.X_result.a.data(), Xe.a.data(), Xe.a.size()), dU = max_abs_diff(p.U_result.a.data(), Ue.a.data(), Ue.a.size());
    printf("east road framed: pick %d (unframed %d), max|dX| %.3g, max|dU| %.3g\n", best, want, dX, dU);
    if (best != want || !(dX <= 1e-9) || !(dU <= 1e-9) || p.last_frames.size() != (size_t)B * CILQR_FRAME_DOUBLES) return 1;

    iLQR q(params, 0, M, B);
    q.set_global_plan(north);
    q.set_Obstacle(obs_n);
    q.set_path_frame(true);
    const int bn = q.run_candidates(egos_n);
    const double dUn = max_abs_diff(q.U_result.a.data(), Ue.a.data(), Ue.a.size()), dXn = turned_diff(q.X_result, Xe),
                 dRn = q.ref_traj_result.cols == Re.cols ? turned_diff(q.ref_traj_result, Re) : INFINITY;
    printf("north road framed: pick %d, max|dU| %.3g against the east road, X against the east plan turned %.3g, ref_traj %.3g, phi %.17g info %d\n",
           bn, dUn, dXn, dRn, q.last_frames[4], (int)q.last_frame_info[0]);
    if (bn != want || !(dUn <= 1e-9) || !(dXn <= 1e-9) || !(dRn <= 1e-9)) return 1;
    if (std::fabs(q.last_frames[4] - kHalfPi) > 1e-15 || q.last_frame_info[0] != 0 || q.last_frame_info.size() != (size_t)B) return 1;
    Un = q.U_result;

    iLQR u(params, 0, M, B);  // the same road without the setter: not the east plan
    u.set_global_plan(north);
    u.set_Obstacle(obs_n);
    u.run_candidates(egos_n);
    const double dUu = max_abs_diff(u.U_result.a.data(), Ue.a.data(), Ue.a.size());
    printf("north road unframed: max|dU| %.3g against the east road\n", dUu);
    if (!(dUu > 1e-6)) { printf("the scene does not show the heading dependence\n"); return 1; }
  }
  // 4. MinTotalCost and run_step
  {
    iLQR a(params, 0, M, B), b(params, 0, M, B);
    a.set_global_plan(east); a.set_Obstacle(obs_e); a.set_candidate_pick(CandidatePick::MinTotalCost, 1.0);
    b.set_global_plan(north); b.set_Obstacle(obs_n); b.set_candidate_pick(CandidatePick::MinTotalCost, 1.0);
    b.set_path_frame(true);
    const int pa = a.run_candidates(egos_e), pb = b.run_candidates(egos_n);
    const double dU = max_abs_diff(b.U_result.a.data(), a.U_result.a.data(), a.U_result.a.size());
    const double dS = a.last_scores.size() == b.last_scores.size() ? max_abs_diff(a.last_scores.data(), b.last_scores.data(), a.last_scores.size()) : INFINITY;
    printf("MinTotalCost: picks %d / %d, max|dU| %.3g, max|d score| %.3g\n", pa, pb, dU, dS);
    if (pa != pb || !(dU <= 1e-9) || !(dS <= 1e-6)) return 1;

    iLQR s(params, 0, M, B), t(params, 0, M, B);
    s.set_global_plan(east); s.set_Obstacle(obs_e);
    t.set_global_plan(north); t.set_Obstacle(obs_n); t.set_path_frame(true);
    s.run_step(&egos_e[4 * 3]);
    t.run_step(&egos_n[4 * 3]);
    const double dUs = max_abs_diff(t.U_result.a.data(), s.U_result.a.data(), s.U_result.a.size()), dXs = turned_diff(t.X_result, s.X_result);
    printf("run_step: max|dU| %.3g, X against the east plan turned %.3g, iterations %d / %d\n", dUs, dXs, s.last_iterations, t.last_iterations);
    if (!(dUs <= 1e-9) || !(dXs <= 1e-9) || s.last_iterations != t.last_iterations || t.last_frames.size() != CILQR_FRAME_DOUBLES) return 1;
  }
  // 5. an in-block mode and the setter
  {
    iLQR p(params, 0, M, B);
    p.set_global_plan(east);
    p.set_Obstacle(obs_e);
    p.set_footprint_check(0.0, INFINITY);
    p.set_path_frame(true);
    if (!throws_logic_error([&] { p.run_candidates(egos_e); }, "set_path_frame")) { printf("footprint check + set_path_frame did not throw\n"); return 1; }
    p.set_path_frame(false);
    if (p.run_candidates(egos_e) < 0) { printf("setter off again: no pick\n"); return 1; }
  }
  printf("path frame ok\n");
  return 0;
}
