// candidates_map_clearance.cpp — iLQR::run_candidates with the map clearance check (set_map_clearance_check) as the last gate: the six
// candidates of candidates_map_tightened.cpp, x0 = (0, -1 + 0.4 b, 4, 0) beside a straight path, NO obstacle, and an uncertainty map
// with one blob at (6, -1.4) — the configuration of the live node, where the map is all the planner knows and the footprint check's
// min_clearance has nothing to act on.  Seeds are the cells above kThreshold = 80.  The constants below are asserted from the CPU
// oracle's solves and the restated clearance in tests/test_map_clearance.py.
//   1. the default pick alone takes the cheapest candidate by J, kPickCheapest, which passes 0.18 m from the blob's occupied cells;
//   2. with set_map_clearance_check(0.0, ...) every candidate whose rectangle stays off the seeds is clear and the pick is still
//      kPickCheapest; last_map_clearance and last_map_step_clearance equal, bit for bit, the rows of a hand-written solve ->
//      cilqr_map_clearance of the same candidates, and the pick is the host-side minimum over that call's total;
//   3. at min_clearance kBetween = 0.25, between the clearances of candidates 3 and 4, the pick moves to the cheapest of those clear,
//      kPickClear;
//   4. at min_clearance 0.5 every candidate is rejected: -1, and the results stay;
//   5. behind the footprint check (both on) the rows are the same and the pick is the hand-written chain's;
//   6. switched off, and with no map set, the run is what it was and the fields are empty.
// Prints "clearances: ..." and "map clearance pick ok" on success.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

int main() {
  const int N = 25, B = 6, kPickCheapest = 3, kPickClear = 4;
  const double kThreshold = 80.0, kReach = 1.0, kBetween = 0.25, inf = INFINITY;
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
  map.layer.resize((size_t)g.rows * g.cols);
  const double x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res);
  const double c = std::cos(kMapPose[2]), s = std::sin(kMapPose[2]);
  for (int j = 0; j < g.cols; ++j)
    for (int i = 0; i < g.rows; ++i) {
      const double mx = x_first - i * g.res, my = y_first - j * g.res;
      const double wx = kMapPose[0] + c * mx - s * my, wy = kMapPose[1] + s * mx + c * my;
      const double r2 = (wx - kBlob[0]) * (wx - kBlob[0]) + (wy - kBlob[1]) * (wy - kBlob[1]);
      map.layer[(size_t)j * g.rows + i] = (float)(100.0 * std::tanh(1.3 * std::exp(-0.5 * r2 / (kBlob[2] * kBlob[2]))));
    }

  // by hand: the same pre-step and solve with the map set, the clearance call on top of J, and behind a footprint check
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, B, N, 0, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<double> poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2), U = default_controls(B, N), X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B);
  std::vector<double> mc((size_t)B * CILQR_MAP_CLEARANCE_FIELDS), clr((size_t)B * N), zero(B), between(B), half(B), fp((size_t)B * CILQR_FOOTPRINT_FIELDS),
      fp_total(B), chained(B), scratch_mc(mc.size()), scratch_clr(clr.size());
  const cilqr_uncertainty_map original = abi_map(map);
  if (cilqr_set_uncertainty_map(h, &original) != CILQR_OK ||
      cilqr_local_plan_batch(h, B, path.cols, path.a.data(), 0, egos.data(), poly.data(), fl.data(), nullptr, nullptr) != CILQR_OK ||
      cilqr_solve_batch(h, B, N, 0, egos.data(), U.data(), poly.data(), fl.data(), nullptr, nullptr, nullptr, X.data(), J.data(), iters.data(), status.data(),
                        CILQR_FLAG_NONE) != CILQR_OK ||
      cilqr_map_clearance(h, B, N, 1, X.data(), 0.0, kThreshold, kReach, 0.0, 0u, J.data(), mc.data(), clr.data(), zero.data()) != CILQR_OK ||
      cilqr_map_clearance(h, B, N, 1, X.data(), 0.0, kThreshold, kReach, kBetween, 0u, J.data(), scratch_mc.data(), scratch_clr.data(), between.data()) != CILQR_OK ||
      cilqr_map_clearance(h, B, N, 1, X.data(), 0.0, kThreshold, kReach, 0.5, 0u, J.data(), scratch_mc.data(), scratch_clr.data(), half.data()) != CILQR_OK ||
      cilqr_footprint_check(h, B, N, 0, 1, X.data(), nullptr, 0.0, 0.0, inf, 0u, J.data(), fp.data(), nullptr, nullptr, fp_total.data()) != CILQR_OK ||
      cilqr_map_clearance(h, B, N, 1, X.data(), 0.0, kThreshold, kReach, kBetween, 0u, fp_total.data(), scratch_mc.data(), scratch_clr.data(), chained.data()) != CILQR_OK) {
    printf("by hand: %s\n", cilqr_last_error());
    return 1;
  }
  cilqr_destroy(h);
  printf("clearances:");
  for (int b = 0; b < B; ++b) printf(" %.9f", mc[(size_t)b * CILQR_MAP_CLEARANCE_FIELDS + CILQR_MC_CLEARANCE]);
  printf("\nJ:");
  for (int b = 0; b < B; ++b) printf(" %.9f", J[b]);
  printf("\n");
  if (first_minimum(J) != kPickCheapest || first_minimum(zero) != kPickCheapest || count_nan(zero) != 2 || first_minimum(between) != kPickClear ||
      count_nan(between) != 4 || first_minimum(half) != -1 || first_minimum(chained) != kPickClear) {
    printf("by hand: the scene is not the one the constants were taken from (picks %d %d %d %d)\n", first_minimum(J), first_minimum(zero), first_minimum(between),
           first_minimum(half));
    return 1;
  }

  const auto fresh = [&](iLQR& q, bool with_map = true) {
    q.set_global_plan(path);
    if (with_map) q.set_uncertainty_map(map);
  };
  // 1. without the check: the cheapest candidate, whatever its distance to the blob
  {
    iLQR q(params, 0, 0, B);
    fresh(q);
    const int best = q.run_candidates(egos);
    if (best != kPickCheapest || !q.last_map_clearance.empty()) { printf("no check: picked %d, the cheapest is %d\n", best, kPickCheapest); return 1; }
  }
  // 2. the check at min_clearance 0: the rows of the hand-written call
  {
    iLQR q(params, 0, 0, B);
    fresh(q);
    q.set_map_clearance_check(0.0, kReach, kThreshold);
    const int best = q.run_candidates(egos);
    if (best != kPickCheapest) { printf("min_clearance 0: picked %d, not %d\n", best, kPickCheapest); return 1; }
    if (!same(q.last_map_clearance, mc) || !same(q.last_map_step_clearance, clr)) { printf("last_map_clearance differs from cilqr_map_clearance on the same solves\n"); return 1; }
    if (!same(q.X_result.a.data(), &X[(size_t)best * 4 * (N + 1)], 4 * (size_t)(N + 1))) { printf("the pick's X differs from the hand-written solve\n"); return 1; }
  }
  // 3. between candidates 3 and 4; 4. nobody is half a metre clear (a rejected run leaves the results as they were)
  {
    iLQR q(params, 0, 0, B);
    fresh(q);
    q.set_map_clearance_check(kBetween, kReach, kThreshold);
    const int best = q.run_candidates(egos);
    if (best != kPickClear || !same(q.last_map_step_clearance, clr)) { printf("min_clearance %.2f: picked %d, the cheapest of those clear is %d\n", kBetween, best, kPickClear); return 1; }
    const Matrix X_before = q.X_result;
    q.set_map_clearance_check(0.5, kReach, kThreshold);
    if (q.run_candidates(egos) != -1 || q.last_map_clearance.size() != mc.size() || !same(q.X_result.a, X_before.a)) { printf("min_clearance 0.5: a plan was picked\n"); return 1; }
  }
  // 5. behind the footprint check
  {
    iLQR q(params, 0, 0, B);
    fresh(q);
    q.set_footprint_check(0.0, inf);
    q.set_map_clearance_check(kBetween, kReach, kThreshold);
    const int best = q.run_candidates(egos);
    if (best != first_minimum(chained) || !same(q.last_footprint, fp) || !same(q.last_map_step_clearance, clr)) { printf("behind the footprint check: picked %d, by hand %d\n", best, first_minimum(chained)); return 1; }
  }
  // 6. switched off; and on with no map set
  {
    iLQR q(params, 0, 0, B);
    fresh(q);
    q.set_map_clearance_check(kBetween, kReach, kThreshold);
    q.set_map_clearance_check(kBetween, kReach, kThreshold, 0.0, false, false);
    int best = q.run_candidates(egos);
    if (best != kPickCheapest || !q.last_map_clearance.empty()) { printf("switched off: picked %d\n", best); return 1; }
    iLQR bare(params, 0, 0, B);
    fresh(bare, false);
    bare.set_map_clearance_check(kBetween, kReach, kThreshold);
    best = bare.run_candidates(egos);
    if (best < 0 || !bare.last_map_clearance.empty() || !bare.last_map_step_clearance.empty()) { printf("no map set: the check ran (%d)\n", best); return 1; }
  }
  // a reach that is negative is refused by the setter
  {
    iLQR q(params, 0, 0, B);
    bool refused = false;
    try { q.set_map_clearance_check(0.0, -1.0, kThreshold); } catch (const std::runtime_error&) { refused = true; }
    if (!refused) { printf("a negative reach was accepted\n"); return 1; }
  }
  printf("map clearance pick ok\n");
  return 0;
}
