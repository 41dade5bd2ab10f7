// replay_main.cpp — ROS-free replay of recorded planner ticks through the adapter: what the node's
// odomCallback does per odometry message (I/ilqr_uncertainty_node.cpp:111-130: set_global_plan → set_Obstacle → run_step →
// publishExperimentData), fed from a text log instead of ROS topics.
//
//   cilqr_replay <log> [device] [--tighten eps[,rounds]] [--stop-fallback d1[,d2...][:hold]] [--map-obstacles thr,gap,min_cells,max_size]
//                [--map-tracker dt,q,r,gate2,min_hits,max_misses] [--clear-movers v_clear,halo[,fill]] [--path-frame]   → one line per tick on stdout
//
// --path-frame: every tick runs under iLQR::set_path_frame(true): the pre-step, the obstacles and the map pose in a frame along the
// tick's slice of the path, X back in the map frame; the line then ends with " frame <phi> <info>" (the frame's heading and its
// CILQR_FRAME_* bits).  Not together with --tighten or --stop-fallback, whose stages are not framed.
//
// --tighten: every tick's solve is followed by `rounds` (default 1) rounds of chance-constraint tightening
// (iLQR::set_chance_tightening) at a chance eps per obstacle entry, under the node's pose noise Sigma0 = diag(0.16^2, 0.16^2, 0,
// 0.017^2) and no process noise; the line then ends with " tighten <max da> <max db> <entry> <capped> <CR_STEP_RISK before>" when
// the tick has obstacles.
//
// --stop-fallback: every tick runs as ONE candidate of iLQR::run_candidates under set_footprint_check(0, +inf) — the exact rectangle
// test against the tick's obstacles — and set_stop_fallback with the braking levels d1, d2 ... (m/s^2) and `hold` (default 1); the line
// then ends with " stop <plan> <level> <pick>": plan 1 when the published plan is a stop plan, 0 when it is the solved one, -1 when the
// tick has no plan at all (X and U are then the tick's before); level its level index or -1; pick the stop pick's row or -1.
//
// --map-obstacles: iLQR::set_map_obstacles(thr, gap, min_cells, max_size, pad 0, K = 16): on every tick that carries a `map` record
// the occupied cells of its layer (value > thr) are clustered into boxes, which are installed behind the tick's obstacles; the line
// then ends with " map_obstacles <installed> <components>".  A tick without a map record clears the map (0 0).
//
// --map-tracker (with --map-obstacles): iLQR::set_map_tracker with 16 slots: the boxes are followed across the ticks by a constant-velocity
// Kalman filter — dt seconds between ticks, Q built for dt from the white-acceleration intensity q (q dt^3/3, q dt^2/2, q dt per axis),
// R = r^2 I, P_birth = diag(r^2, r^2, 16, 16), v_min 0.5 m/s, theta_var_slow 1 — and the confirmed tracks reach the solve predicted over
// the horizon, in place of the standing boxes.  The line then ends with " tracks <n>" and per confirmed track " <id> <x> <y> <speed>
// <heading>".  The ticks must carry no obstacles of their own.
//
// --clear-movers (with --map-tracker): iLQR::set_mover_clearing(v_clear m/s, halo m, fill — default 0): on every tick that carries a map
// the cells of the components that confirmed tracks at v_clear or faster own, and a halo around them, are taken out of the layer before
// the solve reads it.  The line then ends with " clear_movers" and the eight fields of cilqr_clear_movers (movers, cleared, owned linked,
// owned halo, largest value, its cell, contested, kept unknown).
//
// Log (whitespace-separated, '#' starts a comment line):
//   cilqr-replay 1
//   horizon <N>
//   path <P>            followed by P lines "x y"                       (nav_msgs/Path of the global plan)
//   tick                one per odometry message, each followed by
//   ego <x> <y> <v> <theta>
//   obstacles <M>       followed by M lines "x y v theta length width" (held over the horizon, as the node's static-obstacle
//                       callback replicates them, I/ilqr_uncertainty_node.cpp:175-185)
//   map <len_x> <len_y> <res> <pos_x> <pos_y> <pose_x> <pose_y> <pose_theta> <n>      optional; followed by n lines "i j value": the cells
//                       of the layer that are not 0 (the lidar layer of the map node, vehicle frame geometry, the pose it was made at)
// Output per tick: "experiment <start_pos 4> <planning_time> <iterations> <exit> <J> X <4(N+1) values> U <2N values>" —
// X and U in the vehiclepub/Experiment flattening (:243-284).
#include <chrono>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "ilqr_adapter.h"

using namespace cilqr_host;

namespace {

struct Tokens {
  std::vector<std::string> t;
  size_t at = 0;
  explicit Tokens(std::istream& in) {
    std::string line, w;
    while (std::getline(in, line)) {
      const size_t h = line.find_first_not_of(" \t");
      if (h == std::string::npos || line[h] == '#') continue;
      std::istringstream ls(line);
      while (ls >> w) t.push_back(w);
    }
  }
  bool done() const { return at >= t.size(); }
  std::string word() {
    if (done()) throw std::runtime_error("replay log ends in the middle of a record");
    return t[at++];
  }
  void expect(const char* w) {
    const std::string g = word();
    if (g != w) throw std::runtime_error("replay log: expected '" + std::string(w) + "', found '" + g + "'");
  }
  double num() { return std::stod(word()); }
  int integer() { return std::stoi(word()); }
};

}  // namespace

int main(int argc, char** argv) {
  std::vector<const char*> pos;  // the log and the device; options may stand anywhere
  const char *tighten = nullptr, *stop = nullptr, *map_obstacles = nullptr, *map_tracker = nullptr, *clear_movers = nullptr;
  bool path_frame = false;
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "--tighten") == 0 && i + 1 < argc) tighten = argv[++i];
    else if (strcmp(argv[i], "--stop-fallback") == 0 && i + 1 < argc) stop = argv[++i];
    else if (strcmp(argv[i], "--map-obstacles") == 0 && i + 1 < argc) map_obstacles = argv[++i];
    else if (strcmp(argv[i], "--map-tracker") == 0 && i + 1 < argc) map_tracker = argv[++i];
    else if (strcmp(argv[i], "--clear-movers") == 0 && i + 1 < argc) clear_movers = argv[++i];
    else if (strcmp(argv[i], "--path-frame") == 0) path_frame = true;
    else if (strncmp(argv[i], "--", 2) == 0) pos.clear(), i = argc;
    else pos.push_back(argv[i]);
  }
  if (pos.empty() || pos.size() > 2) {
    fprintf(stderr, "usage: %s <log> [device] [--tighten eps[,rounds]] [--stop-fallback d1[,d2...][:hold]] [--map-obstacles thr,gap,min_cells,max_size] [--map-tracker dt,q,r,gate2,min_hits,max_misses] [--clear-movers v_clear,halo[,fill]] [--path-frame]\n", argv[0]);
    return 2;
  }
  try {
    std::ifstream f(pos[0]);
    if (!f) throw std::runtime_error(std::string("cannot open ") + pos[0]);
    Tokens in(f);
    in.expect("cilqr-replay");
    if (in.integer() != 1) throw std::runtime_error("replay log: unknown version");
    in.expect("horizon");
    const int N = in.integer();
    in.expect("path");
    const int P = in.integer();
    if (N < 1 || P < 1) throw std::runtime_error("replay log: horizon and path length must be positive");
    Matrix path(2, P);
    for (int i = 0; i < P; ++i) { path(0, i) = in.num(); path(1, i) = in.num(); }

    Parameters params = default_parameters();
    params.horizon = N;
    std::vector<double> levels;
    int hold = 1;
    if (stop) {
      const char* q = stop;
      for (;;) {
        char* rest = nullptr;
        const double d = strtod(q, &rest);
        if (rest == q) throw std::runtime_error("--stop-fallback takes d1[,d2...][:hold]");
        levels.push_back(d);
        q = rest;
        if (*q != ',') break;
        ++q;
      }
      if (*q == ':') hold = atoi(q + 1);
      else if (*q != 0) throw std::runtime_error("--stop-fallback takes d1[,d2...][:hold]");
    }
    iLQR planner(params, pos.size() > 1 ? atoi(pos[1]) : 0, map_obstacles ? 64 + 16 : 64, stop ? (int)levels.size() : 1);
    if (stop) {
      planner.set_footprint_check(0.0, INFINITY);
      planner.set_stop_fallback(levels, hold);
    }
    if (path_frame) planner.set_path_frame(true);
    if (tighten) {
      char* rest = nullptr;
      const double eps = strtod(tighten, &rest);
      const int rounds = *rest == ',' ? atoi(rest + 1) : 1;
      if (rest == tighten || (*rest != ',' && *rest != 0)) throw std::runtime_error("--tighten takes eps[,rounds]");
      double Sigma0[16] = {};
      Sigma0[0] = Sigma0[5] = 0.16 * 0.16;
      Sigma0[15] = 0.017 * 0.017;
      planner.set_chance_tightening(Sigma0, nullptr, eps, rounds);
    }
    if (map_obstacles) {
      double thr = 0.0, gap = 0.0, max_size = 0.0;
      int min_cells = 0;
      if (sscanf(map_obstacles, "%lf,%lf,%d,%lf", &thr, &gap, &min_cells, &max_size) != 4) throw std::runtime_error("--map-obstacles takes thr,gap,min_cells,max_size");
      planner.set_map_obstacles(thr, gap, min_cells, max_size, 0.0, 16);
    }
    if (map_tracker) {
      if (!map_obstacles) throw std::runtime_error("--map-tracker needs --map-obstacles");
      cilqr_track_filter tf{};
      double q = 0.0, r = 0.0;
      if (sscanf(map_tracker, "%lf,%lf,%lf,%lf,%d,%d", &tf.dt, &q, &r, &tf.gate2, &tf.min_hits, &tf.max_misses) != 6)
        throw std::runtime_error("--map-tracker takes dt,q,r,gate2,min_hits,max_misses");
      const double dt = tf.dt;
      for (int a = 0; a < 2; ++a) {  // column-major, row <= column
        tf.Q[a + 4 * a] = q * dt * dt * dt / 3.0;
        tf.Q[a + 4 * (a + 2)] = q * dt * dt / 2.0;
        tf.Q[(a + 2) + 4 * (a + 2)] = q * dt;
        tf.R[a + 2 * a] = r * r;
        tf.P_birth[a + 4 * a] = r * r;
        tf.P_birth[(a + 2) + 4 * (a + 2)] = 16.0;
      }
      tf.v_min = 0.5;
      tf.theta_var_slow = 1.0;
      planner.set_map_tracker(tf, 16);
    }
    if (clear_movers) {
      if (!map_tracker) throw std::runtime_error("--clear-movers needs --map-tracker");
      double v_clear = 0.0, halo = 0.0, fill = 0.0;
      if (sscanf(clear_movers, "%lf,%lf,%lf", &v_clear, &halo, &fill) < 2) throw std::runtime_error("--clear-movers takes v_clear,halo[,fill]");
      planner.set_mover_clearing(v_clear, halo, (float)fill);
    }
    bool map_on = false;
    while (!in.done()) {
      in.expect("tick");
      in.expect("ego");
      double ego[4];
      for (double& v : ego) v = in.num();
      in.expect("obstacles");
      const int M = in.integer();
      std::vector<Obstacle> obstacles;
      for (int o = 0; o < M; ++o) {
        double rec[6];
        for (double& v : rec) v = in.num();
        Matrix dim(2, N), pose(4, N);
        for (int t = 0; t < N; ++t) {
          for (int r = 0; r < 4; ++r) pose(r, t) = rec[r];
          dim(0, t) = rec[4];
          dim(1, t) = rec[5];
        }
        obstacles.emplace_back(params, dim, pose);
      }
      planner.set_global_plan(path);
      if (map_tracker) {
        if (M) throw std::runtime_error("--map-tracker: the tracker is the one producer of obstacles, and the tick carries its own");
      } else if (M) planner.set_Obstacle(obstacles);
      else planner.clear_Obstacle();
      if (!in.done() && in.t[in.at] == "map") {
        in.expect("map");
        double v[8];
        for (double& x : v) x = in.num();
        Uncertainty um;
        if (cilqr_map_geom_set(&um.geom, v[0], v[1], v[2], v[3], v[4]) != CILQR_OK) throw std::runtime_error(std::string("replay log: map: ") + cilqr_last_error());
        um.pose_x = v[5]; um.pose_y = v[6]; um.pose_theta = v[7];
        um.layer.assign((size_t)um.geom.rows * um.geom.cols, 0.0f);
        for (int n = in.integer(); n > 0; --n) {
          const int i = in.integer(), j = in.integer();
          const double value = in.num();
          if (i < 0 || i >= um.geom.rows || j < 0 || j >= um.geom.cols) throw std::runtime_error("replay log: map cell outside the layer");
          um.layer[(size_t)j * um.geom.rows + i] = (float)value;
        }
        planner.set_uncertainty_map(um);
        map_on = true;
      } else if (map_on) {
        planner.clear_uncertainty_map();
        map_on = false;
      }
      const auto t0 = std::chrono::high_resolution_clock::now();
      int picked = 0;
      if (stop) picked = planner.run_candidates(std::vector<double>(ego, ego + 4));
      else planner.run_step(ego);
      const double secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
      const Experiment e = flatten_experiment(ego, secs, planner.X_result, planner.U_result);
      printf("experiment %.17g %.17g %.17g %.17g %.9g %d %d %.17g X", e.start_pos[0], e.start_pos[1], e.start_pos[2], e.start_pos[3],
             e.planning_time, planner.last_iterations, planner.last_exit, planner.last_cost);
      for (double v : e.X) printf(" %.17g", v);
      printf(" U");
      for (double v : e.U) printf(" %.17g", v);
      if (!planner.last_tighten.empty())
        printf(" tighten %.17g %.17g %d %d %.17g", planner.last_tighten[CILQR_TG_MAX_DA], planner.last_tighten[CILQR_TG_MAX_DB],
               (int)planner.last_tighten[CILQR_TG_MAX_ENTRY], (int)planner.last_tighten[CILQR_TG_CAPPED], planner.last_tighten_risk_before[0]);
      if (map_obstacles) printf(" map_obstacles %d %d", planner.last_map_obstacle_counts[2], planner.last_map_obstacle_counts[0]);
      if (map_tracker) {
        printf(" tracks %d", (int)(planner.last_tracks.size() / 8));
        for (size_t k = 0; k + 8 <= planner.last_tracks.size(); k += 8)
          printf(" %d %.9g %.9g %.9g %.9g", (int)planner.last_tracks[k], planner.last_tracks[k + 1], planner.last_tracks[k + 2], planner.last_tracks[k + 3], planner.last_tracks[k + 4]);
      }
      if (clear_movers) {
        printf(" clear_movers");
        for (double v : planner.last_mover_clearing) printf(" %.9g", v);
      }
      if (path_frame && !planner.last_frames.empty()) printf(" frame %.17g %d", planner.last_frames[4], (int)planner.last_frame_info[0]);
      if (stop) printf(" stop %d %d %d", picked < 0 ? -1 : planner.last_stop_level >= 0 ? 1 : 0, planner.last_stop_level, planner.last_stop_pick);
      printf("\n");
    }
  } catch (const std::exception& ex) {
    fprintf(stderr, "cilqr_replay: %s\n", ex.what());
    return 1;
  }
  return 0;
}
