// candidates_clear_movers.cpp — iLQR::set_mover_clearing: the live node's configuration (no obstacle given, the occupied cells of the
// map are all the planner knows) with a vehicle that CROSSES the road ahead.  A 150 x 100 map of 0.1 m cells centred at (12, 0); an
// 8 x 8-cell block that stands; a 9 x 20-cell block, a two-cell ring of value 30 around it, that moves 5 cells per map towards -y
// (5 m/s at dt = 0.1) and after six maps stands dead ahead at (10.05, 0); four candidates at y = 0, -0.8, -1.6, -2.4 m and 5 m/s
// beside a straight path.  tests/test_clear_movers.py restates the same scene on the CPU.
//   1. by hand, on a handle whose arena holds the map: per map cilqr_map_distance -> cilqr_map_obstacles -> cilqr_track_update ->
//      cilqr_clear_movers in the tracker form (min_hits of the filter, v_clear 1 m/s, halo2 = 9, fill 0); the confirmed rows, compacted
//      in slot order, are what a caller would hand to set_tracked_obstacles;
//   2. under set_map_obstacles + set_map_tracker + set_mover_clearing(1.0, 0.31) the same six set_uncertainty_map calls leave
//      last_mover_clearing equal to the by-hand fields bit for bit;
//   3. run_candidates under set_footprint_check: with the clearing off the block stands in the map over the whole horizon and the
//      pick is the original-map pick (not candidate 0); with it on candidate 0 is picked, and the run equals, bit for bit, a planner
//      that never heard of the clearing and got the by-hand cleared layer through set_uncertainty_map and the by-hand rows through
//      set_tracked_obstacles;
//   4. on = false puts the layer as given back: a run then equals the run of a planner that never had the clearing on;
//      clear_uncertainty_map zeroes the fields;
//   5. the setter without set_map_tracker throws std::logic_error, and so does switching the tracker off under it; a negative v_clear,
//      a halo beyond the limit at the map's resolution and an infinite fill throw std::runtime_error.
// Prints "fields: <8 values>" per map, "pick off: <b>", "pick on: <b>", and "mover clearing ok" on success.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 30, B = 4, K = 8, SLOTS = 8, MAPS = 6;

struct Result {
  int pick;
  Matrix X, U;
  double cost;
  std::vector<double> fp, clearance;
};
Result run(iLQR& p, const std::vector<double>& egos) {
  Result r;
  r.pick = p.run_candidates(egos);
  r.X = p.X_result; r.U = p.U_result; r.cost = p.last_cost; r.fp = p.last_footprint; r.clearance = p.last_footprint_clearance;
  return r;
}
bool equal(const Result& a, const Result& b) {
  return a.pick == b.pick && same(a.X.a, b.X.a) && same(a.U.a, b.U.a) && same(&a.cost, &b.cost, 1) && same(a.fp, b.fp) && same(a.clearance, b.clearance);
}
template <class E, class F>
bool throws(F&& f) {
  try { f(); } catch (const E&) { return true; } catch (...) { return false; }
  return false;
}
}  // namespace

int main() {
  const double kThreshold = 50.0, inf = INFINITY, kVClear = 1.0, kHalo = 0.31;  // (0.3 / 0.1 is just below 3 in doubles: floor((halo/res)^2) would be 8)
  const int kHalo2 = 9;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, 0.0, -0.8, 5.0);
  cilqr_track_filter tf{};
  tf.dt = 0.1;
  for (int a = 0; a < 2; ++a) {
    tf.Q[a + 4 * a] = 0.5 * 0.1 * 0.1 * 0.1 / 3.0; tf.Q[a + 4 * (a + 2)] = 0.5 * 0.1 * 0.1 / 2.0; tf.Q[(a + 2) + 4 * (a + 2)] = 0.5 * 0.1;
    tf.R[a + 2 * a] = 0.05 * 0.05;
    tf.P_birth[a + 4 * a] = 0.05 * 0.05; tf.P_birth[(a + 2) + 4 * (a + 2)] = 16.0;
  }
  tf.gate2 = 9.21; tf.v_min = 1.0; tf.theta_var_slow = 0.25; tf.min_hits = 2; tf.max_misses = 3;

  std::vector<Uncertainty> maps(MAPS);
  for (int k = 0; k < MAPS; ++k) {
    Uncertainty& m = maps[k];
    if (cilqr_map_geom_set(&m.geom, 15.0, 10.0, 0.1, 12.0, 0.0) != CILQR_OK || m.geom.rows != 150 || m.geom.cols != 100) return 1;
    const int rows = m.geom.rows;
    m.layer.assign((size_t)rows * m.geom.cols, 0.0f);
    for (int j = 13 + 5 * k; j < 37 + 5 * k; ++j)
      for (int i = 88; i < 101; ++i) m.layer[(size_t)j * rows + i] = 30.0f;
    for (int j = 15 + 5 * k; j < 35 + 5 * k; ++j)
      for (int i = 90; i < 99; ++i) m.layer[(size_t)j * rows + i] = 100.0f;
    for (int j = 1; j < 9; ++j)
      for (int i = 2; i < 10; ++i) m.layer[(size_t)j * rows + i] = 100.0f;
  }
  const cilqr_map_geom g = maps[0].geom;
  const size_t cells = (size_t)g.rows * g.cols;

  // 1. by hand
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, 64, N, K, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<int32_t> d2(cells), work(cells), label(cells), n_out(4), assign(K);
  std::vector<double> comp((size_t)K * CILQR_MAP_OBSTACLE_FIELDS), boxes((size_t)K * 5);
  std::vector<double> state((size_t)SLOTS * CILQR_TRACK_STATE), world(CILQR_TRACK_WORLD_FIELDS), track((size_t)SLOTS * 6), dim((size_t)SLOTS * 2), cov((size_t)SLOTS * 16);
  std::vector<std::vector<double>> hand_fields(MAPS, std::vector<double>(CILQR_CLEAR_MOVERS_FIELDS));
  std::vector<float> cleared(cells);
  std::vector<double> tracks, dims, covs;
  const double pose0[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < MAPS; ++k) {
    if (cilqr_map_distance(h, 1, maps[k].layer.data(), 0, &g, kThreshold, 0u, d2.data(), nullptr) != CILQR_OK ||
        cilqr_map_obstacles(h, 1, d2.data(), &g, 0, 0u, pose0, 0, K, 1, inf, 0.0, work.data(), label.data(), n_out.data(), comp.data(), boxes.data(),
                            nullptr, nullptr) != CILQR_OK ||
        cilqr_track_update(h, 1, SLOTS, K, boxes.data(), n_out.data() + 2, 4, &tf, state.data(), state.data(), world.data(),
                           k == 0 ? CILQR_TRACK_RESET : 0u, assign.data(), track.data(), dim.data(), cov.data()) != CILQR_OK ||
        cilqr_clear_movers(h, 1, maps[k].layer.data(), 0, &g, label.data(), K, comp.data(), SLOTS, assign.data(), state.data(), tf.min_hits, kVClear,
                           nullptr, kHalo2, 0.0f, cleared.data(), nullptr, hand_fields[k].data()) != CILQR_OK) {
      printf("by hand, map %d: %s\n", k, cilqr_last_error());
      return 1;
    }
    if (n_out[2] != 2) { printf("by hand, map %d: %d rows, the scene has two blocks\n", k, n_out[2]); return 1; }
    tracks.clear(); dims.clear(); covs.clear();
    for (int m = 0; m < SLOTS; ++m) {
      const double* row = &state[(size_t)m * CILQR_TRACK_STATE];
      if (!(row[CILQR_TS_ID] >= 0.0 && row[CILQR_TS_HITS] >= tf.min_hits)) continue;
      tracks.insert(tracks.end(), &track[6 * m], &track[6 * m] + 6);
      dims.insert(dims.end(), &dim[2 * m], &dim[2 * m] + 2);
      covs.insert(covs.end(), &cov[16 * m], &cov[16 * m] + 16);
    }
  }
  cilqr_destroy(h);
  if (hand_fields[MAPS - 1][CILQR_CM_MOVERS] != 1.0 || hand_fields[MAPS - 1][CILQR_CM_CLEARED] != 312.0) {
    printf("by hand: %g movers, %g cells cleared after the last map\n", hand_fields[MAPS - 1][CILQR_CM_MOVERS], hand_fields[MAPS - 1][CILQR_CM_CLEARED]);
    return 1;
  }

  // 2. the clearing on the facade
  iLQR on(params, 0, K, B), off(params, 0, K, B), by_hand(params, 0, K, B);
  for (iLQR* p : {&on, &off, &by_hand}) {
    p->set_global_plan(path);
    p->set_footprint_check(0.0, kThreshold);
  }
  for (iLQR* p : {&on, &off}) {
    p->set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
    p->set_map_tracker(tf, SLOTS);
  }
  on.set_mover_clearing(kVClear, kHalo);
  for (int k = 0; k < MAPS; ++k) {
    on.set_uncertainty_map(maps[k]);
    off.set_uncertainty_map(maps[k]);
    printf("fields:");
    for (double v : on.last_mover_clearing) printf(" %.17g", v);
    printf("\n");
    if (!same(on.last_mover_clearing, hand_fields[k].data(), CILQR_CLEAR_MOVERS_FIELDS)) { printf("map %d: last_mover_clearing differs from cilqr_clear_movers by hand\n", k); return 1; }
    if (!same(on.last_tracks, off.last_tracks)) { printf("map %d: the clearing changed the tracks\n", k); return 1; }
    for (double v : off.last_mover_clearing)
      if (v != 0.0) { printf("map %d: fields without the setter\n", k); return 1; }
  }

  // 3. the two picks, and the C-ABI sequence by hand
  Uncertainty hand_map = maps[MAPS - 1];
  hand_map.layer = cleared;
  by_hand.set_uncertainty_map(hand_map);
  by_hand.set_tracked_obstacles(tracks, dims, covs, {});
  const Result r_on = run(on, egos), r_off = run(off, egos), r_hand = run(by_hand, egos);
  printf("pick off: %d\npick on: %d\n", r_off.pick, r_on.pick);
  printf("map hit steps off:");
  for (int b = 0; b < B; ++b) printf(" %g", r_off.fp[(size_t)CILQR_FOOTPRINT_FIELDS * b + CILQR_FP_MAP_HIT_STEPS]);
  printf("\nmap hit steps on:");
  for (int b = 0; b < B; ++b) printf(" %g", r_on.fp[(size_t)CILQR_FOOTPRINT_FIELDS * b + CILQR_FP_MAP_HIT_STEPS]);
  printf("\n");
  if (!equal(r_on, r_hand)) { printf("the run under the clearing differs from the by-hand cleared layer and rows (picks %d, %d)\n", r_on.pick, r_hand.pick); return 1; }
  if (r_on.pick != 0 || r_off.pick == 0) { printf("picks: on %d (want 0), off %d (want another, or -1)\n", r_on.pick, r_off.pick); return 1; }
  if (r_off.fp[CILQR_FP_MAP_HIT_STEPS] == 0.0 || r_on.fp[CILQR_FP_MAP_HIT_STEPS] != 0.0) { printf("candidate 0 against the block: the map hits are not what the scene is for\n"); return 1; }

  // 4. off again; the map cleared
  {
    iLQR touched(params, 0, K, B), never(params, 0, K, B);
    for (iLQR* p : {&touched, &never}) {
      p->set_global_plan(path);
      p->set_footprint_check(0.0, kThreshold);
      p->set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
      p->set_map_tracker(tf, SLOTS);
    }
    touched.set_mover_clearing(kVClear, kHalo);
    for (int k = 0; k < MAPS; ++k) {
      touched.set_uncertainty_map(maps[k]);
      never.set_uncertainty_map(maps[k]);
    }
    touched.set_mover_clearing(kVClear, kHalo, 0.0f, false);
    for (double v : touched.last_mover_clearing)
      if (v != 0.0) { printf("on = false left fields\n"); return 1; }
    const Result rt = run(touched, egos), rn = run(never, egos);
    if (!equal(rt, rn) || !equal(rn, r_off)) { printf("clearing off: the run differs from a planner that never had it on (picks %d, %d)\n", rt.pick, rn.pick); return 1; }
    touched.set_mover_clearing(kVClear, kHalo);  // (with a map set: the clearing runs on it at once)
    if (!same(touched.last_mover_clearing, hand_fields[MAPS - 1].data(), CILQR_CLEAR_MOVERS_FIELDS)) { printf("on again: the fields differ\n"); return 1; }
    touched.clear_uncertainty_map();
    for (double v : touched.last_mover_clearing)
      if (v != 0.0) { printf("clear_uncertainty_map left fields\n"); return 1; }
  }

  // 5. what the setter needs, and its limits
  {
    iLQR q(params, 0, K, B);
    if (!throws_logic_error([&] { q.set_mover_clearing(kVClear, kHalo); }, "set_map_tracker")) { printf("the clearing without set_map_tracker was accepted\n"); return 1; }
    q.set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
    if (!throws_logic_error([&] { q.set_mover_clearing(kVClear, kHalo); }, "set_map_tracker")) { printf("the clearing without set_map_tracker was accepted\n"); return 1; }
    printf("setter without a tracker throws\n");
    q.set_map_tracker(tf, SLOTS);
    if (!throws<std::runtime_error>([&] { q.set_mover_clearing(-1.0, kHalo); }) || !throws<std::runtime_error>([&] { q.set_mover_clearing(NAN, kHalo); }) ||
        !throws<std::runtime_error>([&] { q.set_mover_clearing(kVClear, -0.1); }) || !throws<std::runtime_error>([&] { q.set_mover_clearing(kVClear, inf); }) ||
        !throws<std::runtime_error>([&] { q.set_mover_clearing(kVClear, kHalo, INFINITY); })) {
      printf("a bad v_clear, halo or fill was accepted\n");
      return 1;
    }
    q.set_uncertainty_map(maps[0]);
    if (!throws<std::runtime_error>([&] { q.set_mover_clearing(kVClear, 3.3); })) { printf("a halo of 33 cells was accepted\n"); return 1; }
    q.set_mover_clearing(kVClear, 3.2001, NAN);  // 32 cells: the limit; a NaN fill
    if (!throws_logic_error([&] { q.set_map_tracker(tf, SLOTS, false); }, "set_mover_clearing")) { printf("the tracker went off under the clearing\n"); return 1; }
  }
  printf("mover clearing ok\n");
  return 0;
}
