// candidates_stop.cpp — iLQR::run_candidates under set_stop_fallback: scene W of tests/test_stop_plans.py in its obstacle variant.  Four
// candidates x0 = (0, 0.3 b, 5, 0) beside a straight path, horizon 40, one obstacle rectangle 0.5 m long and 8 m wide standing
// across the whole road at x = kWall.  The solver drives through it (asserted from the CPU oracle's solves in
// tests/test_stop_plans.py), so set_footprint_check(0, +inf) rejects every solved candidate; braked at 1.5 m/s^2 a plan still reaches
// the wall, at 3 and 5 m/s^2 it stops clear.  Against the C-ABI sequence called by hand — pre-step, solve, footprint check (S = 1),
// cilqr_stop_plans, footprint check (S = D, base = the rows' cost), the minimum on the host — bit for bit:
//   1. with the setter off the run returns -1 and leaves X_result, U_result and the stop fields untouched;
//   2. with it on the run returns the candidate and level the hand-called sequence picks, X_result / U_result are that row, last_stop
//      and last_stop_footprint are the sequence's rows, and the warm start stays: the same run again gives the same bits;
//   3. with the wall out of reach a solved candidate passes: the index, X_result, U_result, every other last_* field and the next run
//      (the warm start) equal those of a planner without the setter, last_stop_level is -1 and last_stop is filled;
//   4. with the wall 3 m ahead every level is blocked: -1, last_stop_pick -1;
//   5. more than floor(max_candidates / D) candidates throws; without set_footprint_check the run throws std::logic_error naming it.
// Prints "stop pick: candidate c level l" and "stop fallback ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {

const int N = 40, M = 1, B = 4, D = 3, R = B * D;
const double kLevels[D] = {1.5, 3.0, 5.0}, kWeight = 1.0e6, kMaxDeviation = 0.5, inf = INFINITY;
const int kHold = 1;

struct ByHand {
  std::vector<double> X, U, J, fp, total, Xs, Us, sp, cost, sfp, stotal;
  int pick = -1, stop_pick = -1;
};

// the C-ABI sequence on a handle of its own; false (and a message) when a call fails
bool by_hand(const Parameters& params, const Matrix& path, const std::vector<double>& egos, double wall, ByHand& o) {
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, R, N, M, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return false; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), clr((size_t)B * N);
  std::vector<int32_t> iters(B), status(B);
  o.U = default_controls(B, N);
  o.X.assign((size_t)B * 4 * (N + 1), 0.0); o.J.assign(B, 0.0); o.fp.assign((size_t)B * CILQR_FOOTPRINT_FIELDS, 0.0); o.total.assign(B, 0.0);
  o.Xs.assign((size_t)R * 4 * (N + 1), 0.0); o.Us.assign((size_t)R * 2 * N, 0.0); o.sp.assign((size_t)R * CILQR_STOP_FIELDS, 0.0); o.cost.assign(R, 0.0);
  o.sfp.assign((size_t)R * CILQR_FOOTPRINT_FIELDS, 0.0); o.stotal.assign(R, 0.0);
  const double pose1[4] = {wall, 0.0, 0.0, 0.0}, dim1[2] = {0.5, 8.0};
  const cilqr_obstacles obs{pose1, dim1, nullptr, 0, 1, 0, 0};
  const bool ok =
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
      cilqr_solve_batch_obstacles(h, B, N, M, egos.data(), o.U.data(), poly.data(), fl.data(), &obs, o.X.data(), o.J.data(), iters.data(), status.data(),
                                  CILQR_FLAG_NONE) == CILQR_OK &&
      cilqr_footprint_check(h, B, N, M, 1, o.X.data(), &obs, 0.0, 0.0, inf, 0u, o.J.data(), o.fp.data(), clr.data(), nullptr, o.total.data()) == CILQR_OK &&
      cilqr_stop_plans(h, B, N, D, o.X.data(), o.U.data(), kLevels, kHold, kMaxDeviation, o.J.data(), kWeight, 0u, o.Xs.data(), o.Us.data(), o.sp.data(),
                       o.cost.data()) == CILQR_OK &&
      cilqr_footprint_check(h, B, N, M, D, o.Xs.data(), &obs, 0.0, 0.0, inf, 0u, o.cost.data(), o.sfp.data(), nullptr, nullptr, o.stotal.data()) == CILQR_OK;
  if (!ok) printf("by hand: %s\n", cilqr_last_error());
  cilqr_destroy(h);
  o.pick = first_minimum(o.total);
  o.stop_pick = first_minimum(o.stotal);
  return ok;
}

void dress(iLQR& q, const Parameters& params, const Matrix& path, double wall, bool fallback) {
  q.set_global_plan(path);
  q.set_Obstacle(std::vector<Obstacle>{standing_obstacle(params, N, wall, 0.0, 0.0, 0.5, 8.0)});
  q.set_footprint_check(0.0, inf);
  if (fallback) q.set_stop_fallback(std::vector<double>(kLevels, kLevels + D), kHold, kMaxDeviation);
}

}  // namespace

int main() {
  const double kWall = 9.25, kFar = 60.0, kNear = 3.0;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, 0.0, 0.3);

  ByHand w, far, near;
  if (!by_hand(params, path, egos, kWall, w) || !by_hand(params, path, egos, kFar, far) || !by_hand(params, path, egos, kNear, near)) return 1;
  // the scene is the one the constants were taken from
  bool scene = w.pick == -1 && w.stop_pick >= 0 && far.pick >= 0 && near.pick == -1 && near.stop_pick == -1;
  for (int b = 0; b < B; ++b) scene = scene && w.stotal[(size_t)b * D] != w.stotal[(size_t)b * D] && w.stotal[(size_t)b * D + 1] == w.stotal[(size_t)b * D + 1] &&
                                    w.stotal[(size_t)b * D + 2] == w.stotal[(size_t)b * D + 2];
  if (!scene || w.stop_pick % D != 1) {
    printf("by hand: the scene is not the one the constants were taken from (picks %d %d, far %d, near %d %d)\n", w.pick, w.stop_pick, far.pick, near.pick, near.stop_pick);
    return 1;
  }
  printf("stop pick: candidate %d level %d\n", w.stop_pick / D, w.stop_pick % D);

  // 1. the setter off: no plan, nothing touched
  {
    iLQR q(params, 0, M, R);
    dress(q, params, path, kWall, false);
    const Matrix X_before = q.X_result, U_before = q.U_result;
    if (q.run_candidates(egos) != -1 || !same(q.X_result.a, X_before.a) || !same(q.U_result.a, U_before.a) || !q.last_stop.empty() ||
        !q.last_stop_footprint.empty() || q.last_stop_level != -1 || q.last_stop_pick != -1 || !same(q.last_footprint, w.fp)) {
      printf("setter off: the run did not return -1 with everything untouched\n");
      return 1;
    }
  }
  // 2. the setter on: the hand-called pick and row; the warm start stays
  {
    iLQR q(params, 0, M, R);
    dress(q, params, path, kWall, true);
    for (int run = 0; run < 2; ++run) {
      const int best = q.run_candidates(egos);
      const size_t row = (size_t)w.stop_pick;
      if (best != w.stop_pick / D || q.last_stop_level != w.stop_pick % D || q.last_stop_pick != w.stop_pick) {
        printf("setter on, run %d: returned %d level %d pick %d, by hand row %d\n", run, best, q.last_stop_level, q.last_stop_pick, w.stop_pick);
        return 1;
      }
      if (!same(q.X_result.a.data(), &w.Xs[row * 4 * (N + 1)], 4 * (size_t)(N + 1)) || q.X_result.a.size() != 4 * (size_t)(N + 1) ||
          !same(q.U_result.a.data(), &w.Us[row * 2 * N], 2 * (size_t)N) || q.U_result.a.size() != 2 * (size_t)N) {
        printf("setter on, run %d: X_result / U_result are not the hand-called stop row\n", run);
        return 1;
      }
      if (!same(q.last_stop, w.sp) || !same(q.last_stop_footprint, w.sfp) || !same(q.last_footprint, w.fp)) {
        printf("setter on, run %d: last_stop / last_stop_footprint / last_footprint differ from the hand-called sequence\n", run);
        return 1;
      }
    }
  }
  // 3. a solved candidate passes: everything is what it is without the setter
  {
    iLQR a(params, 0, M, R), b(params, 0, M, R);
    dress(a, params, path, kFar, false);
    dress(b, params, path, kFar, true);
    for (int run = 0; run < 2; ++run) {  // (the second run starts from the first one's warm start)
      const int ia = a.run_candidates(egos), ib = b.run_candidates(egos);
      if (ia != ib || (run == 0 && ia != far.pick) || !same(a.X_result.a, b.X_result.a) || !same(a.U_result.a, b.U_result.a) ||
          !same(a.ref_traj_result.a, b.ref_traj_result.a) || !same(a.last_footprint, b.last_footprint) ||
          !same(a.last_footprint_clearance, b.last_footprint_clearance) || !same(a.last_scores, b.last_scores) || a.last_iterations != b.last_iterations ||
          a.last_exit != b.last_exit || !same(&a.last_cost, &b.last_cost, 1)) {
        printf("a passing scene, run %d: the run under the setter differs from the run without it (%d, %d)\n", run, ia, ib);
        return 1;
      }
      if (b.last_stop_level != -1 || b.last_stop.size() != (size_t)R * CILQR_STOP_FIELDS || b.last_stop_footprint.size() != (size_t)R * CILQR_FOOTPRINT_FIELDS ||
          !a.last_stop.empty()) {
        printf("a passing scene, run %d: last_stop_level %d, last_stop of %zu values\n", run, b.last_stop_level, b.last_stop.size());
        return 1;
      }
      if (run == 0 && (!same(b.last_stop, far.sp) || b.last_stop_pick != far.stop_pick)) { printf("a passing scene: last_stop differs from the hand-called rows\n"); return 1; }
    }
  }
  // 4. every level blocked
  {
    iLQR q(params, 0, M, R);
    dress(q, params, path, kNear, true);
    if (q.run_candidates(egos) != -1 || q.last_stop_pick != -1 || q.last_stop_level != -1 || !same(q.last_stop, near.sp)) {
      printf("every level blocked: a plan was published\n");
      return 1;
    }
  }
  // 5. the limits
  {
    iLQR q(params, 0, M, R);
    dress(q, params, path, kWall, true);
    bool thrown = false;
    try { q.run_candidates(spread_egos(B + 1, 0.0, 0.3)); } catch (const std::logic_error&) { thrown = false; } catch (const std::runtime_error& e) { thrown = strstr(e.what(), "max_candidates") != nullptr; }
    if (!thrown) { printf("%d candidates at %d levels on %d rows did not throw\n", B + 1, D, R); return 1; }
    if (q.run_candidates(egos) != w.stop_pick / D) { printf("after the refused run the planner no longer answers\n"); return 1; }
    iLQR bare(params, 0, M, R);
    bare.set_global_plan(path);
    bare.set_stop_fallback(std::vector<double>(kLevels, kLevels + D), kHold, kMaxDeviation);
    if (!throws_logic_error([&] { bare.run_candidates(egos); }, "set_footprint_check")) { printf("without set_footprint_check the run did not throw\n"); return 1; }
    iLQR sampled(params, 0, 4, R);
    dress(sampled, params, path, kWall, true);
    Draws draws;
    sampled.set_obstacle_samples(make_pose_samples(2, draws), 2);
    if (!throws_logic_error([&] { sampled.run_candidates(egos); }, "set_footprint_check")) { printf("with set_obstacle_samples the run did not throw\n"); return 1; }
  }
  printf("stop fallback ok\n");
  return 0;
}
