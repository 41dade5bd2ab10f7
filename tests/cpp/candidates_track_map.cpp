// candidates_track_map.cpp — iLQR::set_track_map: the scene of tests/test_rasterize_tracks.py's purpose test.  A straight path, two
// candidates at y = 0 and -0.4 m and 5 m/s, N = 40, w_uncertainty 5, a zero 150 x 60 map at 0.2 m in front of the ego, two tracked
// vehicles that cross x = 20 heading +y at 5 m/s (4 x 2 m, P_0 = diag(0.3^2, 0.3^2, 0.5^2, 0.05^2), Q = diag(1e-4, 1e-4, 4e-4, 1e-6)).
//   usage: candidates_track_map DUMP
//   1. ellipses off (the live node's configuration): run_candidates against the C-ABI sequence called by hand — predict, local plan,
//      solve with M = 0, rasterise along the plans (host form), each candidate's layer set, re-solve from the plan's U — bit for bit:
//      the pick, X_result, U_result, last_cost, last_track_map.  The first plans, the layers and the re-solved plans go to DUMP for the
//      restated pipeline of the test.
//   2. ellipses on: the same with M = 2 in both solves.
//   3. after a run the handle holds the original map: debug_map_cost at the plan's states equals, bit for bit, that of a planner that
//      only had the map set.
//   4. run_step equals run_candidates with that one candidate.
//   5. rounds = 0, no tracks, or no map: the results are, bit for bit, those of a planner that never heard of set_track_map.
//   6. beside set_map_tightening one round is gains and covariance chain -> rasterise -> cilqr_tighten_map on the RASTERISED layers ->
//      one re-solve: against that sequence by hand, bit for bit, with last_track_map and last_tighten_map.
//   7. ellipses off with set_pose_covariance_check and set_obstacle_covariance_check behind it: the plan is made through the map only and
//      judged by cilqr_chance_risk_cov against the tracks: last_chance_risk and the pick against the sequence by hand.
//   8. round counts that disagree and set_chance_tightening beside ellipses = false throw std::logic_error; bad arguments throw
//      std::runtime_error.
// Prints "ellipses off ok", "ellipses on ok", "map restored ok", "run_step ok", "off switches ok", "composed with map tightening ok",
// "judged behind the map ok", "conflicts throw ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "facade_common.h"

using namespace cilqr_host;

namespace {
const int N = 40, M = 2, B = 2;
const double kInflate = 0.2, kZ = 2.0;
const int kWindow = 2;


struct Scene {
  Parameters params;
  Matrix path{2, 200};
  std::vector<double> egos, tracks, dims, P0, Q;
  Uncertainty map;
};

const double kEps = 0.05, kCap = 1.0;
const double kMaxRisk = 0.561;  // between the two candidates' CR_STEP_RISK after the round (0.5626 and 0.5595 on the CPU, tests/test_rasterize_tracks.py)

struct ByHand {
  std::vector<double> X1, U1, X2, U2, J2, fields, tm, risk, total;
  std::vector<float> layers;
  std::vector<int32_t> iters;
  int best = -1;
};

// The C-ABI sequence by hand, host forms, for the candidates egos[0 .. nb): one round.
// tighten: the composed round of set_map_tightening (Sigma0 = sigma0, W = Q).  judge: cilqr_chance_risk_cov on the final plans.
bool by_hand(const Scene& sc, const double* egos, int nb, bool ellipses, ByHand& o, bool tighten = false, bool judge = false,
             const double* sigma0 = nullptr, const double* W = nullptr) {
  cilqr_handle* h = nullptr;
  // (max_batch 64: the host form of the rasteriser stages nb layers of 9000 floats through the arena)
  if (cilqr_create(&sc.params, 64, N, M, 0, &h) != CILQR_OK) return false;
  const size_t cells = sc.map.layer.size();
  std::vector<double> pose((size_t)M * 4 * N), dim((size_t)M * 2 * N), cov((size_t)M * 3 * N), poly((size_t)nb * CILQR_POLY_COEFFS), fl((size_t)nb * 2),
      U = default_controls(nb, N), J(nb);
  std::vector<int32_t> status(nb);
  o.X1.assign((size_t)nb * 4 * (N + 1), 0.0); o.X2 = o.X1; o.J2.assign(nb, 0.0); o.iters.assign(nb, 0);
  o.fields.assign((size_t)nb * CILQR_TRACK_MAP_FIELDS, 0.0); o.layers.assign((size_t)nb * cells, 0.0f);
  const cilqr_obstacles obs{pose.data(), dim.data(), nullptr, 0, N, 1, 0};
  const int Ms = ellipses ? M : 0;
  const cilqr_uncertainty_map original = abi_map(sc.map, sc.map.layer.data(), 0);
  bool ok = cilqr_predict_obstacles(h, 1, N, M, sc.tracks.data(), sc.dims.data(), sc.P0.data(), sc.Q.data(), pose.data(), dim.data(), cov.data(),
                                    nullptr) == CILQR_OK &&
            cilqr_set_uncertainty_map(h, &original) == CILQR_OK &&
            cilqr_local_plan_batch(h, nb, sc.path.cols, sc.path.a.data(), 0, egos, poly.data(), fl.data(), nullptr, nullptr) == CILQR_OK &&
            cilqr_solve_batch_obstacles(h, nb, N, Ms, egos, U.data(), poly.data(), fl.data(), Ms ? &obs : nullptr, o.X1.data(), J.data(),
                                        o.iters.data(), status.data(), CILQR_FLAG_NONE) == CILQR_OK;
  o.U1 = U;
  std::vector<double> k((size_t)nb * 2 * N), K((size_t)nb * 8 * N), sigma((size_t)nb * (N + 1) * 16), trisk((size_t)nb * CILQR_CHANCE_FIELDS);
  std::vector<int32_t> gok(nb);
  std::vector<float> tight((size_t)nb * cells);
  o.tm.assign((size_t)nb * CILQR_TIGHTEN_MAP_FIELDS, 0.0);
  if (tighten)
    ok = ok && cilqr_gains_batch(h, nb, N, M, o.X1.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), gok.data()) == CILQR_OK &&
         cilqr_chance_risk(h, nb, N, M, o.X1.data(), U.data(), K.data(), sigma0, 0, W, &obs, 0u, 1.0, nullptr, trisk.data(), nullptr, nullptr,
                           sigma.data(), nullptr) == CILQR_OK;
  ok = ok && cilqr_rasterize_tracks(h, nb, N, M, o.X1.data(), &obs, cov.data(), kInflate, kZ, kWindow, 0u, o.layers.data(), o.fields.data()) == CILQR_OK;
  // (the host form of the setter takes one layer: each candidate is re-solved alone against its own — a solve depends on its own inputs alone)
  for (int b = 0; ok && b < nb; ++b) {
    cilqr_uncertainty_map own = abi_map(sc.map, &o.layers[(size_t)b * cells], 0);
    if (tighten) {  // the tightening reads the candidate's RASTERISED layer
      ok = cilqr_set_uncertainty_map(h, &own) == CILQR_OK &&
           cilqr_tighten_map(h, 1, N, &o.X1[(size_t)b * 4 * (N + 1)], &sigma[(size_t)b * (N + 1) * 16], cilqr_chance_kappa(kEps), kCap,
                             &tight[(size_t)b * cells], &o.tm[(size_t)b * CILQR_TIGHTEN_MAP_FIELDS]) == CILQR_OK;
      own = abi_map(sc.map, &tight[(size_t)b * cells], 0);
      if (!ok) break;
    }
    ok = cilqr_set_uncertainty_map(h, &own) == CILQR_OK &&
         cilqr_solve_batch_obstacles(h, 1, N, Ms, egos + 4 * b, &U[(size_t)b * 2 * N], &poly[(size_t)b * CILQR_POLY_COEFFS], &fl[(size_t)b * 2],
                                     Ms ? &obs : nullptr, &o.X2[(size_t)b * 4 * (N + 1)], &o.J2[b], &o.iters[b], &status[b], CILQR_FLAG_NONE) == CILQR_OK;
  }
  o.U2 = U;
  if (ok && judge) {  // against the tracks themselves, with their covariance, and the original map on the handle
    o.risk.assign((size_t)nb * CILQR_CHANCE_FIELDS, 0.0); o.total.assign(nb, 0.0);
    std::vector<double> step((size_t)nb * N);
    ok = cilqr_set_uncertainty_map(h, &original) == CILQR_OK &&
         cilqr_gains_batch(h, nb, N, M, o.X2.data(), U.data(), poly.data(), fl.data(), &obs, 1.0, k.data(), K.data(), gok.data()) == CILQR_OK &&
         cilqr_chance_risk_cov(h, nb, N, M, o.X2.data(), U.data(), K.data(), sigma0, 0, W, &obs, cov.data(), 0u, kMaxRisk, o.J2.data(),
                               o.risk.data(), step.data(), nullptr, nullptr, o.total.data()) == CILQR_OK;
  }
  if (!ok) printf("the sequence by hand failed: %s\n", cilqr_last_error());
  o.best = -1;
  const std::vector<double>& rank = judge ? o.total : o.J2;
  for (int b = 0; b < nb; ++b)
    if (rank[b] == rank[b] && (o.best < 0 || rank[b] < rank[o.best])) o.best = b;
  cilqr_destroy(h);
  return ok;
}

bool pick_equals(const iLQR& p, int pick, const ByHand& o, const char* what) {
  if (pick != o.best || pick < 0) { printf("%s: pick %d, by hand %d\n", what, pick, o.best); return false; }
  if (!same(p.X_result.a.data(), &o.X2[(size_t)pick * 4 * (N + 1)], 4 * (size_t)(N + 1)) || !same(p.U_result.a.data(), &o.U2[(size_t)pick * 2 * N], 2 * (size_t)N) ||
      !same(&p.last_cost, &o.J2[pick], 1)) { printf("%s: the pick's plan differs from the sequence by hand\n", what); return false; }
  if (!same(p.last_track_map, o.fields)) { printf("%s: last_track_map differs from cilqr_rasterize_tracks by hand\n", what); return false; }
  return true;
}

void setup(iLQR& p, const Scene& sc, bool tracks = true, bool map = true) {
  p.set_global_plan(sc.path);
  if (tracks) p.set_tracked_obstacles(sc.tracks, sc.dims, sc.P0, sc.Q);
  if (map) p.set_uncertainty_map(sc.map);
}

void dump(const char* path, const Scene& sc, const ByHand& o) {
  FILE* f = fopen(path, "w");
  if (!f) return;
  fprintf(f, "%d %d %d %d %d\n", B, N, sc.map.geom.rows, sc.map.geom.cols, o.best);
  for (const std::vector<double>* v : {&o.X1, &o.U1, &o.X2, &o.U2, &o.J2, &o.fields})
    for (double x : *v) fprintf(f, "%.17g\n", x);
  for (int32_t i : o.iters) fprintf(f, "%d\n", i);
  for (float v : o.layers) fprintf(f, "%.9g\n", (double)v);
  fclose(f);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: candidates_track_map DUMP\n"); return 2; }
  Scene sc;
  sc.params = default_parameters();
  sc.params.horizon = N;
  sc.params.safe_length = 1.1; sc.params.safe_width = 0.9;
  sc.params.w_uncertainty = 5.0;
  sc.path = straight_path();
  for (int b = 0; b < B; ++b) { const double e[4] = {0.0, -0.4 * b, 5.0, 0.0}; sc.egos.insert(sc.egos.end(), e, e + 4); }
  const double half_pi = 1.57079632679489655800;
  sc.tracks = {20.0, -10.0, 5.0, half_pi, 0.0, 0.0, 20.0, -22.0, 5.0, half_pi, 0.0, 0.0};
  sc.dims = {4.0, 2.0, 4.0, 2.0};
  sc.P0.assign(32, 0.0);
  for (int m = 0; m < M; ++m) { double* P = &sc.P0[(size_t)16 * m]; P[0] = 0.3 * 0.3; P[5] = 0.3 * 0.3; P[10] = 0.5 * 0.5; P[15] = 0.05 * 0.05; }
  sc.Q.assign(16, 0.0);
  sc.Q[0] = 1e-4; sc.Q[5] = 1e-4; sc.Q[10] = 4e-4; sc.Q[15] = 1e-6;
  if (cilqr_map_geom_set(&sc.map.geom, 30.0, 12.0, 0.2, 15.0, 0.0) != CILQR_OK) return 1;
  sc.map.pose_x = 0.0; sc.map.pose_y = 0.0; sc.map.pose_theta = 0.0;
  sc.map.probes_l = 3; sc.map.probes_w = 3;
  sc.map.layer.assign((size_t)sc.map.geom.rows * sc.map.geom.cols, 0.0f);

  // ---- 1: ellipses off
  ByHand off;
  if (!by_hand(sc, sc.egos.data(), B, false, off)) return 1;
  iLQR p_off(sc.params, 0, M, B);
  setup(p_off, sc);
  p_off.set_track_map(kInflate, kZ, kWindow, 1, false);
  const int pick_off = p_off.run_candidates(sc.egos);
  if (!pick_equals(p_off, pick_off, off, "ellipses off")) return 1;
  for (int b = 0; b < B; ++b)
    printf("ellipses off, candidate %d: J %.9f, raised %g, largest value %g, iterations %d\n", b, off.J2[b], off.fields[(size_t)6 * b + CILQR_TKM_RAISED],
           off.fields[(size_t)6 * b + CILQR_TKM_MAX_VALUE], off.iters[b]);
  dump(argv[1], sc, off);
  printf("ellipses off ok\n");

  // ---- 2: ellipses on
  ByHand on;
  if (!by_hand(sc, sc.egos.data(), B, true, on)) return 1;
  iLQR p_on(sc.params, 0, M, B);
  setup(p_on, sc);
  p_on.set_track_map(kInflate, kZ, kWindow);
  const int pick_on = p_on.run_candidates(sc.egos);
  if (!pick_equals(p_on, pick_on, on, "ellipses on")) return 1;
  if (same(on.X2, off.X2)) { printf("the ellipses changed nothing\n"); return 1; }
  printf("ellipses on ok\n");

  // ---- 3: the original map is back on the handle
  std::vector<double> states(p_off.X_result.a.begin(), p_off.X_result.a.begin() + 4 * (size_t)N);
  iLQR fresh(sc.params, 0, M, B);
  setup(fresh, sc, false, true);
  if (!same(p_off.debug_map_cost(states), fresh.debug_map_cost(states))) { printf("after the run the handle's map is not the original\n"); return 1; }
  printf("map restored ok\n");

  // ---- 4: run_step is run_candidates with one candidate
  ByHand one;
  if (!by_hand(sc, sc.egos.data(), 1, false, one)) return 1;
  iLQR p_step(sc.params, 0, M, B);
  setup(p_step, sc);
  p_step.set_track_map(kInflate, kZ, kWindow, 1, false);
  p_step.run_step(sc.egos.data());
  if (!same(p_step.X_result.a.data(), one.X2.data(), 4 * (size_t)(N + 1)) || !same(p_step.U_result.a.data(), one.U2.data(), 2 * (size_t)N) ||
      !same(p_step.last_track_map, one.fields) || !same(&p_step.last_cost, &one.J2[0], 1)) { printf("run_step differs from the sequence by hand\n"); return 1; }
  printf("run_step ok\n");

  // ---- 5: the off switches
  iLQR parent(sc.params, 0, M, B), zero(sc.params, 0, M, B), no_map(sc.params, 0, M, B);
  setup(parent, sc);
  setup(zero, sc);
  zero.set_track_map(kInflate, kZ, kWindow, 0);
  setup(no_map, sc, true, false);
  no_map.set_track_map(kInflate, kZ, kWindow);
  iLQR parent_no_map(sc.params, 0, M, B);
  setup(parent_no_map, sc, true, false);
  const int a = parent.run_candidates(sc.egos), z = zero.run_candidates(sc.egos);
  if (a != z || !same(parent.X_result.a, zero.X_result.a) || !same(parent.U_result.a, zero.U_result.a) || !zero.last_track_map.empty()) { printf("rounds = 0 is not off\n"); return 1; }
  const int c = parent_no_map.run_candidates(sc.egos), d = no_map.run_candidates(sc.egos);
  if (c != d || !same(parent_no_map.X_result.a, no_map.X_result.a) || !no_map.last_track_map.empty()) { printf("no map set: the rounds are not skipped\n"); return 1; }
  iLQR no_tracks(sc.params, 0, M, B), parent_no_tracks(sc.params, 0, M, B);
  setup(no_tracks, sc, false, true);
  no_tracks.set_track_map(kInflate, kZ, kWindow, 1, false);
  setup(parent_no_tracks, sc, false, true);
  const int e = parent_no_tracks.run_candidates(sc.egos), f = no_tracks.run_candidates(sc.egos);
  if (e != f || !same(parent_no_tracks.X_result.a, no_tracks.X_result.a) || !no_tracks.last_track_map.empty()) { printf("no tracks set: the rounds are not skipped\n"); return 1; }
  printf("off switches ok\n");

  double sigma0[16] = {};
  sigma0[0] = 0.16 * 0.16; sigma0[5] = 0.16 * 0.16; sigma0[15] = 0.017 * 0.017;

  // ---- 6: composed with the map tightening.  (A process noise of 400 Q: under the plan's gains the tracker's Q leaves a position
  // sigma of a few centimetres at the steps where the tracks are met, less than one 0.2 m cell, and the dilation would reach nothing)
  std::vector<double> Wbig(sc.Q);
  for (double& w : Wbig) w *= 400.0;
  ByHand comp;
  if (!by_hand(sc, sc.egos.data(), B, false, comp, true, false, sigma0, Wbig.data())) return 1;
  iLQR p_comp(sc.params, 0, M, B);
  setup(p_comp, sc);
  p_comp.set_track_map(kInflate, kZ, kWindow, 1, false);
  p_comp.set_map_tightening(sigma0, Wbig.data(), kEps, 1, kCap);
  const int pick_comp = p_comp.run_candidates(sc.egos);
  if (!pick_equals(p_comp, pick_comp, comp, "composed with the map tightening")) return 1;
  if (!same(p_comp.last_tighten_map, comp.tm)) { printf("composed: last_tighten_map differs from cilqr_tighten_map on the rasterised layers\n"); return 1; }
  for (int b = 0; b < B; ++b)
    printf("composed, candidate %d: J %.9f, rasterised %g cells, tightening raised %g more, reach %.3f m\n", b, comp.J2[b],
           comp.fields[(size_t)6 * b + CILQR_TKM_RAISED], comp.tm[(size_t)CILQR_TIGHTEN_MAP_FIELDS * b + CILQR_TM_RAISED],
           comp.tm[(size_t)CILQR_TIGHTEN_MAP_FIELDS * b + CILQR_TM_MAX_REACH]);
  if (same(comp.X2, off.X2)) { printf("composed: the tightening of the rasterised layers changed nothing\n"); return 1; }
  if (!same(p_comp.debug_map_cost(states), fresh.debug_map_cost(states))) { printf("composed: the handle's map is not the original afterwards\n"); return 1; }
  printf("composed with map tightening ok\n");

  // ---- 7: planned through the map only, judged against the tracks
  ByHand judged;
  if (!by_hand(sc, sc.egos.data(), B, false, judged, false, true, sigma0, sc.Q.data())) return 1;
  iLQR p_judged(sc.params, 0, M, B);
  setup(p_judged, sc);
  p_judged.set_track_map(kInflate, kZ, kWindow, 1, false);
  p_judged.set_obstacle_covariance_check(true);
  p_judged.set_pose_covariance_check(sigma0, sc.Q.data(), kMaxRisk);
  const int pick_judged = p_judged.run_candidates(sc.egos);
  if (pick_judged != judged.best || !same(p_judged.last_chance_risk, judged.risk) || !same(p_judged.last_track_map, judged.fields)) {
    printf("judged: pick %d, by hand %d, or the risk rows differ from cilqr_chance_risk_cov by hand\n", pick_judged, judged.best);
    return 1;
  }
  if (!same(judged.X2, off.X2)) { printf("judged: the check changed the plans\n"); return 1; }
  if (pick_judged != 1 || pick_off != 0) { printf("judged: the check was to move the pick from the cheapest candidate, 0, to 1: picks %d and %d\n", pick_off, pick_judged); return 1; }
  for (int b = 0; b < B; ++b)
    printf("judged, candidate %d: CR_STEP_RISK against the tracks %.6f (max_risk %.2f)\n", b, judged.risk[(size_t)CILQR_CHANCE_FIELDS * b + CILQR_CR_STEP_RISK], kMaxRisk);
  printf("judged behind the map ok\n");

  // ---- 8: conflicts and bad arguments
  iLQR both(sc.params, 0, M, B);
  setup(both, sc);
  both.set_track_map(kInflate, kZ, kWindow, 2, false);
  both.set_map_tightening(sigma0, sc.Q.data(), kEps, 1);
  int threw = 0;
  try { both.run_candidates(sc.egos); } catch (const std::logic_error&) { ++threw; }  // 2 rounds beside 1
  both.set_map_tightening(nullptr, nullptr, kEps);
  both.set_track_map(kInflate, kZ, kWindow, 1, false);
  both.set_chance_tightening(sigma0, sc.Q.data(), kEps, 1);
  try { both.run_candidates(sc.egos); } catch (const std::logic_error&) { ++threw; }  // nothing to inflate
  if (threw != 2) { printf("conflicts: %d of 2 threw std::logic_error\n", threw); return 1; }
  int bad = 0;
  const double nan = std::nan("");
  try { both.set_track_map(-1.0, kZ, kWindow); } catch (const std::runtime_error&) { ++bad; }
  try { both.set_track_map(kInflate, nan, kWindow); } catch (const std::runtime_error&) { ++bad; }
  try { both.set_track_map(kInflate, kZ, -1); } catch (const std::runtime_error&) { ++bad; }
  try { both.set_track_map(kInflate, kZ, kWindow, -1); } catch (const std::runtime_error&) { ++bad; }
  if (bad != 4) { printf("bad arguments: %d of 4 threw\n", bad); return 1; }
  printf("conflicts throw ok\n");
  return 0;
}
