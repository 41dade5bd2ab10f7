// facade_common.h — what the facade programs (candidates_*.cpp, step_vs_candidates.cpp, adapter_*.cpp) share: the bit-for-bit
// comparisons, the pick by hand, the fixed draws, the dump writers, and the pieces of the common scene — a straight path, egos spread
// sideways at 5 m/s, vehicle-sized obstacles that stand still, a costmap of smooth bumps.  Each program keeps its own constants, its own
// C-ABI sequence called by hand and its own assertions.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include <vector>

#include "ilqr_adapter.h"

inline bool same(const double* a, const double* b, size_t n) { return memcmp(a, b, n * sizeof(double)) == 0; }
inline bool same(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && same(a.data(), b.data(), a.size()); }
inline bool same_i(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(int32_t)) == 0;
}
inline int first_minimum(const std::vector<double>& v) {  // strict <, NaN never wins; -1: none
  int best = -1;
  for (int b = 0; b < (int)v.size(); ++b)
    if (v[b] == v[b] && (best < 0 || v[b] < v[best])) best = b;
  return best;
}
inline int count_nan(const std::vector<double>& v) {
  int n = 0;
  for (double x : v) n += x != x;
  return n;
}
template <class F>
bool throws_logic_error(F&& f, const char* needle) {  // a std::logic_error whose text names `needle`
  try {
    f();
  } catch (const std::logic_error& e) {
    return strstr(e.what(), needle) != nullptr;
  } catch (...) {
    return false;
  }
  return false;
}

// sums of four uniforms from a fixed linear congruential sequence, scaled to the given sigma
struct Draws {
  uint64_t state = 0x9e3779b97f4a7c15ull;
  double unit() {  // in [-1, 1)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 4503599627370496.0 - 1.0;
  }
  double gauss(double sigma) { return (unit() + unit() + unit() + unit()) * sigma * 0.8660254037844386; }  // var 4/3 -> 1
};
// S ego start offsets (dx, dy, 0, dtheta) of the size of the node's pose noise: the next 12 S units of `draws`
inline std::vector<double> make_offsets(int S, Draws& draws) {
  std::vector<double> d(4 * (size_t)S, 0.0);
  for (int s = 0; s < S; ++s) {
    d[4 * s + 0] = draws.gauss(0.16);
    d[4 * s + 1] = draws.gauss(0.16);
    d[4 * s + 3] = draws.gauss(0.017);
  }
  return d;
}
inline std::vector<double> make_offsets(int S) {
  Draws draws;
  return make_offsets(S, draws);
}
// n obstacle pose samples (dx, dy, dtheta), sigma 0.45 m and 0.05 rad
inline std::vector<double> make_pose_samples(int n, Draws& draws) {
  std::vector<double> d(3 * (size_t)n);
  for (int j = 0; j < n; ++j) {
    d[3 * j + 0] = draws.gauss(0.45);
    d[3 * j + 1] = draws.gauss(0.45);
    d[3 * j + 2] = draws.gauss(0.05);
  }
  return d;
}

inline void put(FILE* f, const std::vector<double>& v) {
  for (double x : v) fprintf(f, "%.17g\n", x);
}
inline void put_i(FILE* f, const std::vector<int32_t>& v) {
  for (int32_t x : v) fprintf(f, "%d\n", (int)x);
}

// The facade's Uncertainty as the C-ABI takes it: its own layer, one for the batch, or `layer` (per solve with a layer_stride).
inline cilqr_uncertainty_map abi_map(const cilqr_host::Uncertainty& u, const float* layer = nullptr, int64_t layer_stride = 0) {
  cilqr_uncertainty_map m{};
  m.layer = layer ? layer : u.layer.data(); m.geom = u.geom;
  m.pose_x = u.pose_x; m.pose_y = u.pose_y; m.pose_theta = u.pose_theta;
  m.layer_stride = layer_stride;
  m.probes_l = u.probes_l; m.probes_w = u.probes_w;
  return m;
}

// The warm start every fresh planner holds (cilqr_default_control_seq), for B candidates: [B][2N]
inline std::vector<double> default_controls(int B, int N) {
  std::vector<double> seq(2 * (size_t)N), U((size_t)B * 2 * N);
  cilqr_default_control_seq(N, seq.data());
  for (int b = 0; b < B; ++b) memcpy(&U[(size_t)b * 2 * N], seq.data(), seq.size() * sizeof(double));
  return U;
}

// ---- the scene ----------------------------------------------------------------------------------------------------------------
inline cilqr_host::Matrix straight_path(int points = 200) {  // along +x, a waypoint per metre
  cilqr_host::Matrix path(2, points);
  for (int i = 0; i < points; ++i) { path(0, i) = 1.0 * i; path(1, i) = 0.0; }
  return path;
}
inline std::vector<double> spread_egos(int B, double y0, double dy, double v = 5.0) {  // at x = 0, heading 0, y = y0 + dy b
  std::vector<double> egos(4 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    egos[4 * b + 0] = 0.0;
    egos[4 * b + 1] = y0 + dy * b;
    egos[4 * b + 2] = v;
    egos[4 * b + 3] = 0.0;
  }
  return egos;
}
// a vehicle standing at (x, y), heading theta, over the horizon
inline cilqr_host::Obstacle standing_obstacle(const cilqr_host::Parameters& params, int N, double x, double y, double theta = 0.0,
                                              double length = 4.79, double width = 2.16) {
  cilqr_host::Matrix dim(2, N), pose(4, N);
  for (int t = 0; t < N; ++t) {
    dim(0, t) = length; dim(1, t) = width;
    pose(0, t) = x; pose(1, t) = y; pose(2, t) = 0.0; pose(3, t) = theta;
  }
  return cilqr_host::Obstacle(params, dim, pose);
}
// M of them in a row ahead, dx apart from x0, alternately y_even and y_odd to the side, each turned 0.1 rad further
inline std::vector<cilqr_host::Obstacle> staggered_obstacles(const cilqr_host::Parameters& params, int N, int M, double x0, double dx,
                                                             double y_even, double y_odd) {
  std::vector<cilqr_host::Obstacle> obstacles;
  for (int o = 0; o < M; ++o) obstacles.push_back(standing_obstacle(params, N, x0 + dx * o, (o % 2) ? y_odd : y_even, 0.1 * o));
  return obstacles;
}
// The costmap of 200 x 80 cells of 0.2 m centred 15 m ahead, map pose 0: cell (i, j) has its centre at (34.9 - 0.2 i, 7.9 - 0.2 j); its
// value is 100 tanh(z / 100), z the sum of the bumps amplitude * exp(-((x - cx)^2 / sx^2 + (y - cy)^2 / sy^2) / 2).
struct Bump { double amplitude, cx, cy, sx, sy; };
const double kBumpGeom[5] = {40.0, 16.0, 0.2, 15.0, 0.0}, kBumpMapPose[3] = {0.0, 0.0, 0.0};  // (what the dumps write)
inline bool bump_costmap(cilqr_host::Uncertainty& um, std::initializer_list<Bump> bumps) {
  if (cilqr_map_geom_set(&um.geom, kBumpGeom[0], kBumpGeom[1], kBumpGeom[2], kBumpGeom[3], kBumpGeom[4]) != CILQR_OK) return false;
  const int rows = um.geom.rows, cols = um.geom.cols;
  um.layer.resize((size_t)rows * cols);
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const double x = 34.9 - 0.2 * i, y = 7.9 - 0.2 * j;
      double z = 0.0;
      for (const Bump& b : bumps) z += b.amplitude * std::exp(-0.5 * (std::pow((x - b.cx) / b.sx, 2) + std::pow((y - b.cy) / b.sy, 2)));
      um.layer[(size_t)j * rows + i] = (float)(100.0 * std::tanh(z / 100.0));
    }
  um.pose_x = kBumpMapPose[0]; um.pose_y = kBumpMapPose[1]; um.pose_theta = kBumpMapPose[2];
  return true;
}
