// candidates_map_tracker.cpp — iLQR::set_map_tracker: the live node's configuration (no obstacle given, the occupied cells of the map
// are all the planner knows) with a vehicle that MOVES.  A 150 x 100 map of 0.1 m cells centred at (12, 0); an 8 x 8-cell block that
// stands and a 20 x 9-cell block that moves 5 cells per map towards the ego (5 m/s at dt = 0.1); four maps; four candidates at
// y = 0, -0.8, -1.6, -2.4 m and 5 m/s beside a straight path.  tests/test_track_update.py restates the same scene on the CPU.
//   1. by hand, on a handle whose arena holds the map: per map cilqr_map_distance -> cilqr_map_obstacles -> cilqr_track_update (the
//      count read from n_out + 2 with stride 4, the table in place, the first with CILQR_TRACK_RESET); the confirmed rows, compacted
//      in slot order, are what a caller would hand to set_tracked_obstacles;
//   2. under set_map_obstacles + set_map_tracker the same four set_uncertainty_map calls leave last_tracks and last_track_counts equal
//      to the by-hand rows and world record bit for bit; one track moves, keeps its ID and has the block's speed;
//   3. run_candidates under set_pose_covariance_check + set_obstacle_covariance_check runs (the judges have their input) and equals,
//      bit for bit, a planner that never heard of the tracker and got the by-hand rows through set_tracked_obstacles (whose own
//      equality with the C-ABI sequence candidates_tracked.cpp shows); the moving track raises the risk of the nearest candidate
//      above what the standing rows of set_map_obstacles alone give;
//   4. with the tracker switched off again a run equals, bit for bit, the run of a planner that never had it on;
//   5. clear_Obstacle makes the next map a first tick; the tracker is the one producer (set_tracked_obstacles, set_Obstacle and
//      set_obstacle_covariance throw std::logic_error, and so does the tracker without set_map_obstacles); K above 64 and slots out of
//      range throw std::runtime_error.
// Prints "track: id x y v theta" of the moving track per map, the candidates' CR_STEP_RISK, and "map tracker ok" on success.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 30, B = 4, K = 8, SLOTS = 8, MAPS = 4;

struct Result {
  int pick;
  Matrix X, U;
  double cost;
  std::vector<double> risk, step;
};
Result run(iLQR& p, const std::vector<double>& egos) {
  Result r;
  r.pick = p.run_candidates(egos);
  r.X = p.X_result; r.U = p.U_result; r.cost = p.last_cost; r.risk = p.last_chance_risk; r.step = p.last_step_risk;
  return r;
}
bool equal(const Result& a, const Result& b) {
  return a.pick == b.pick && same(a.X.a, b.X.a) && same(a.U.a, b.U.a) && same(&a.cost, &b.cost, 1) && same(a.risk, b.risk) && same(a.step, b.step);
}
template <class E, class F>
bool throws(F&& f) {
  try { f(); } catch (const E&) { return true; } catch (...) { return false; }
  return false;
}
}  // namespace

int main() {
  const double kThreshold = 50.0, inf = INFINITY, max_risk = 0.06;
  Parameters params = default_parameters();
  params.horizon = N;
  const Matrix path = straight_path();
  const std::vector<double> egos = spread_egos(B, 0.0, -0.8, 5.0);
  double sigma0[16] = {};
  sigma0[0] = sigma0[5] = 0.16 * 0.16;
  sigma0[15] = 0.017 * 0.017;
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
    m.layer.assign((size_t)m.geom.rows * m.geom.cols, 0.0f);
    for (int j = 1; j < 9; ++j)
      for (int i = 2; i < 10; ++i) m.layer[(size_t)j * m.geom.rows + i] = 100.0f;
    for (int j = 8; j < 17; ++j)
      for (int i = 20 + 5 * k; i < 40 + 5 * k; ++i) m.layer[(size_t)j * m.geom.rows + i] = 100.0f;
  }
  const cilqr_map_geom g = maps[0].geom;
  const size_t cells = (size_t)g.rows * g.cols;

  // 1. by hand
  cilqr_handle* h = nullptr;
  if (cilqr_create(&params, 64, N, K, 0, &h) != CILQR_OK) { printf("cilqr_create: %s\n", cilqr_last_error()); return 1; }
  std::vector<int32_t> d2(cells), work(cells), label(cells), n_out(4), assign(K);
  std::vector<double> comp((size_t)K * CILQR_MAP_OBSTACLE_FIELDS), boxes((size_t)K * 5);
  std::vector<double> state((size_t)SLOTS * CILQR_TRACK_STATE), world(CILQR_TRACK_WORLD_FIELDS), track((size_t)SLOTS * 6), dim((size_t)SLOTS * 2), cov((size_t)SLOTS * 16);
  std::vector<std::vector<double>> hand_rows(MAPS), hand_world(MAPS);
  std::vector<double> tracks, dims, covs;
  const double pose0[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < MAPS; ++k) {
    if (cilqr_map_distance(h, 1, maps[k].layer.data(), 0, &g, kThreshold, 0u, d2.data(), nullptr) != CILQR_OK ||
        cilqr_map_obstacles(h, 1, d2.data(), &g, 0, 0u, pose0, 0, K, 1, inf, 0.0, work.data(), label.data(), n_out.data(), comp.data(), boxes.data(),
                            nullptr, nullptr) != CILQR_OK ||
        cilqr_track_update(h, 1, SLOTS, K, boxes.data(), n_out.data() + 2, 4, &tf, state.data(), state.data(), world.data(),
                           k == 0 ? CILQR_TRACK_RESET : 0u, assign.data(), track.data(), dim.data(), cov.data()) != CILQR_OK) {
      printf("by hand, map %d: %s\n", k, cilqr_last_error());
      return 1;
    }
    if (n_out[2] != 2) { printf("by hand, map %d: %d rows, the scene has two blocks\n", k, n_out[2]); return 1; }
    hand_world[k] = world;
    tracks.clear(); dims.clear(); covs.clear();
    for (int m = 0; m < SLOTS; ++m) {
      const double* row = &state[(size_t)m * CILQR_TRACK_STATE];
      if (!(row[CILQR_TS_ID] >= 0.0 && row[CILQR_TS_HITS] >= tf.min_hits)) continue;
      tracks.insert(tracks.end(), &track[6 * m], &track[6 * m] + 6);
      dims.insert(dims.end(), &dim[2 * m], &dim[2 * m] + 2);
      covs.insert(covs.end(), &cov[16 * m], &cov[16 * m] + 16);
      const double r[8] = {row[CILQR_TS_ID], track[6 * m], track[6 * m + 1], track[6 * m + 2], track[6 * m + 3], dim[2 * m], dim[2 * m + 1], (double)m};
      hand_rows[k].insert(hand_rows[k].end(), r, r + 8);
    }
  }
  cilqr_destroy(h);

  // 2. the tracker on the facade
  iLQR a(params, 0, K, B);
  a.set_global_plan(path);
  a.set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
  a.set_map_tracker(tf, SLOTS);
  double moving_id = -1.0, speed = 0.0;
  for (int k = 0; k < MAPS; ++k) {
    a.set_uncertainty_map(maps[k]);
    if (!same(a.last_tracks, hand_rows[k]) || !same(a.last_track_counts, hand_world[k].data(), CILQR_TRACK_WORLD_FIELDS)) {
      printf("map %d: last_tracks or last_track_counts differ from cilqr_track_update by hand\n", k);
      return 1;
    }
    int movers = 0;
    for (size_t r = 0; r + 8 <= a.last_tracks.size(); r += 8)
      if (a.last_tracks[r + 3] > 0.0) {
        ++movers;
        printf("track: %d %d %.12g %.12g %.12g %.12g\n", k, (int)a.last_tracks[r], a.last_tracks[r + 1], a.last_tracks[r + 2], a.last_tracks[r + 3], a.last_tracks[r + 4]);
        if (moving_id >= 0.0 && a.last_tracks[r] != moving_id) { printf("map %d: the moving track changed its ID\n", k); return 1; }
        moving_id = a.last_tracks[r];
        speed = a.last_tracks[r + 3];
      }
    if (movers != (k == 0 ? 0 : 1)) { printf("map %d: %d moving confirmed tracks\n", k, movers); return 1; }
  }
  if (a.last_tracks.size() != 16 || std::fabs(speed - 5.0) > 0.25) { printf("after %d maps: %zu confirmed rows, speed %.6f\n", MAPS, a.last_tracks.size() / 8, speed); return 1; }

  // 3. the judges that read tracks have their input
  iLQR by_hand(params, 0, K, B), standing(params, 0, K, B);
  for (iLQR* p : {&a, &by_hand, &standing}) {
    p->set_global_plan(path);
    p->set_obstacle_covariance_check(true);
    p->set_pose_covariance_check(sigma0, nullptr, max_risk);
  }
  by_hand.set_uncertainty_map(maps[MAPS - 1]);
  by_hand.set_tracked_obstacles(tracks, dims, covs, {});
  standing.set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
  standing.set_uncertainty_map(maps[MAPS - 1]);
  const Result ra = run(a, egos), rh = run(by_hand, egos), rs = run(standing, egos);
  if (!equal(ra, rh)) { printf("the tracker's run differs from set_tracked_obstacles with the by-hand rows (picks %d, %d)\n", ra.pick, rh.pick); return 1; }
  printf("risk tracked:");
  for (int b = 0; b < B; ++b) printf(" %.12g", ra.risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK]);
  printf("\nrisk standing:");
  for (int b = 0; b < B; ++b) printf(" %.12g", rs.risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK]);
  printf("\npicks: %d %d\n", ra.pick, rs.pick);
  if (!(ra.risk[CILQR_CR_STEP_RISK] > 1e3 * rs.risk[CILQR_CR_STEP_RISK]) || ra.pick < 0) { printf("the moving track does not show in the risk\n"); return 1; }

  // 4. off again: the run of a planner that never had the tracker on
  {
    iLQR touched(params, 0, K, B), never(params, 0, K, B);
    for (iLQR* p : {&touched, &never}) {
      p->set_global_plan(path);
      p->set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
    }
    touched.set_map_tracker(tf, SLOTS);
    touched.set_uncertainty_map(maps[0]);
    touched.set_uncertainty_map(maps[1]);
    touched.set_map_tracker(tf, SLOTS, false);
    if (!touched.last_tracks.empty() || touched.last_map_obstacles.size() != 10) { printf("on = false left tracks, or did not put the rows back\n"); return 1; }
    touched.set_uncertainty_map(maps[MAPS - 1]);
    never.set_uncertainty_map(maps[MAPS - 1]);
    const Result rt = run(touched, egos), rn = run(never, egos);
    if (!equal(rt, rn) || !same(touched.last_map_obstacles, never.last_map_obstacles)) { printf("tracker off: the run differs from a planner that never had it on\n"); return 1; }
  }

  // 5. a first tick again after clear_Obstacle; one producer; limits
  a.clear_Obstacle();
  a.set_uncertainty_map(maps[0]);
  if (a.last_track_counts[CILQR_TW_TICKS] != 1.0 || a.last_track_counts[CILQR_TW_NEXT_ID] != 2.0 || a.last_track_counts[CILQR_TW_BORN] != 2.0 || !a.last_tracks.empty()) {
    printf("clear_Obstacle did not start the tracker over\n");
    return 1;
  }
  if (!throws_logic_error([&] { a.set_tracked_obstacles({20.0, 5.0, 1.0, 0.0, 0.0, 0.0}, {4.0, 2.0}, {}, {}); }, "set_map_tracker") ||
      !throws_logic_error([&] { a.set_Obstacle({standing_obstacle(params, N, 40.0, 30.0)}); }, "set_map_tracker") ||
      !throws_logic_error([&] { a.set_obstacle_covariance({0.1, 0.0, 0.1}); }, "set_map_tracker")) {
    printf("a second producer beside the tracker was accepted\n");
    return 1;
  }
  {
    iLQR q(params, 0, K, B);
    if (!throws_logic_error([&] { q.set_map_tracker(tf, SLOTS); }, "set_map_obstacles")) { printf("the tracker without set_map_obstacles was accepted\n"); return 1; }
    q.set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, K);
    cilqr_track_filter bad = tf;
    bad.dt = 0.0;
    if (!throws<std::runtime_error>([&] { q.set_map_tracker(tf, 0); }) || !throws<std::runtime_error>([&] { q.set_map_tracker(tf, K + 1); }) ||
        !throws<std::runtime_error>([&] { q.set_map_tracker(bad, SLOTS); })) {
      printf("slots out of range or a bad filter were accepted\n");
      return 1;
    }
    q.set_map_tracker(tf, SLOTS);
    if (!throws<std::runtime_error>([&] { q.set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, 65); })) { printf("K = 65 under the tracker was accepted\n"); return 1; }
    iLQR wide(params, 0, 80, B);
    wide.set_map_obstacles(kThreshold, 0.0, 1, inf, 0.0, 65);
    if (!throws<std::runtime_error>([&] { wide.set_map_tracker(tf, SLOTS); })) { printf("the tracker over K = 65 was accepted\n"); return 1; }
  }
  printf("map tracker ok\n");
  return 0;
}
