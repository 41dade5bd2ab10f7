// cilqr_host_plan.h — where the arrays of a host-buffer call lie in the handle's device arena: plain C++, no HIP (checked
// without a GPU by tests/test_host_plan.py through tests/cpp/host_plan_dump.cpp).  cilqr_host_io.cpp moves what a plan names.
//
// A call DECLARES its arrays in order — inputs, then arrays that travel both ways (the U of a solve), then outputs — and each
// gets the next 16-byte-aligned place.  Declared in that order, what travels to the device is one contiguous prefix
// [0, in_end) and what returns one contiguous suffix [out_begin, end): a call small enough for the pinned staging buffer moves
// as ONE copy each way.  Declaring an array swaps the caller's HOST pointer for the array's place in the arena, so after its
// plan_* function a host form holds exactly the pointers its `_device` form takes.  An input of no elements or with a null
// pointer takes no place and becomes null; so does a null output, unless the call keeps its place (the solve's J, iters and
// status, which the kernels and the multi-device argmin use whoever asked for them).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "cilqr.h"

namespace cilqr {

struct HostPlan {
  enum { CAP = 16 };  // (the largest call, the chance risk with obs_cov, declares 14 arrays)
  struct Entry {
    const void* src;  // host source, null: nothing travels in
    void* dst;        // host destination, null: nothing travels back
    size_t off, bytes;
  };
  char* base;  // the arena
  Entry e[CAP];
  int n = 0, phase = 0;
  size_t in_end = 0, out_begin = 0, end = 0;
  bool ok = true;  // false: arrays declared out of order, or more than CAP of them (a mistake in a plan_* function)

  explicit HostPlan(char* arena) : base(arena) {}

  template <typename T> void in(const T*& p, size_t count) { p = (const T*)place(0, p, nullptr, p ? count * sizeof(T) : 0); }
  template <typename T> void inout(T*& p, size_t count) { p = (T*)place(1, p, p, p ? count * sizeof(T) : 0); }
  template <typename T> void out(T*& p, size_t count, bool keep_null = false) { p = (T*)place(2, nullptr, p, p || keep_null ? count * sizeof(T) : 0); }

 private:
  char* place(int ph, const void* src, void* dst, size_t bytes) {
    if (bytes == 0) return nullptr;
    if (ph < phase || n == CAP) { ok = false; return nullptr; }
    phase = ph;
    const size_t at = end;
    e[n++] = Entry{src, dst, at, bytes};
    end = (end + bytes + 15) & ~(size_t)15;
    if (ph == 0) out_begin = end;
    if (ph <= 1) in_end = end;
    return base ? base + at : nullptr;  // (no arena: the plan only gives sizes and offsets)
  }
};

// ---- what each host form declares (B solves, horizon N, M obstacles; every pointer is swapped for its place in the arena) ----

// Obstacles travel as the span of entries their strides address (4 pose + 2 dimension doubles each) and w_span weights.
inline void plan_obstacles(HostPlan& p, size_t M, cilqr_obstacles& o, size_t span, size_t w_span) {
  if (M == 0) { o = cilqr_obstacles{}; return; }
  p.in(o.weight, w_span);
  p.in(o.pose, span * 4);
  p.in(o.dim, span * 2);
}

// cilqr_solve_batch, cilqr_solve_batch_obstacles, cilqr_multi_solve_batch; cilqr_solve_batch_sampled with n_samples > 0, M its
// n_obs and `o` its dense nominal tables without weights.
inline void plan_solve(HostPlan& p, size_t B, size_t N, size_t M, size_t n_samples, const double*& x0, double*& U, const double*& poly,
                       const double*& xplan_fl, cilqr_obstacles& o, size_t span, size_t w_span, const double*& samp_off, double*& X_out,
                       double*& J_out, int32_t*& iters_out, int32_t*& status_out) {
  p.in(x0, B * 4);
  p.in(poly, B * CILQR_POLY_COEFFS);
  p.in(xplan_fl, B * 2);
  plan_obstacles(p, M, o, span, w_span);
  p.in(samp_off, B * M * n_samples * 3);
  p.inout(U, B * 2 * N);
  p.out(X_out, B * 4 * (N + 1));
  p.out(J_out, B, true);
  p.out(iters_out, B, true);
  p.out(status_out, B, true);
}

// cilqr_score_batch; cilqr_score_batch_sampled as above.
inline void plan_score(HostPlan& p, size_t B, size_t N, size_t M, size_t n_samples, const double*& X, const double*& U, const double*& poly,
                       const double*& xplan_fl, cilqr_obstacles& o, size_t span, size_t w_span, const double*& samp_off, double*& score,
                       double*& total) {
  p.in(poly, B * CILQR_POLY_COEFFS);
  p.in(xplan_fl, B * 2);
  plan_obstacles(p, M, o, span, w_span);
  p.in(samp_off, B * M * n_samples * 3);
  p.in(U, B * 2 * N);
  p.in(X, B * 4 * (N + 1));
  p.out(score, B * CILQR_SCORE_FIELDS);
  p.out(total, B);
}

inline void plan_gains(HostPlan& p, size_t B, size_t N, size_t M, const double*& X, const double*& U, const double*& poly,
                       const double*& xplan_fl, cilqr_obstacles& o, size_t span, size_t w_span, double*& k_out, double*& K_out,
                       int32_t*& ok_out) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(poly, B * CILQR_POLY_COEFFS);
  p.in(xplan_fl, B * 2);
  plan_obstacles(p, M, o, span, w_span);
  p.out(k_out, B * 2 * N);
  p.out(K_out, B * 8 * N);
  p.out(ok_out, B);
}

// cilqr_gains_batch_sampled: M its n_obs, `o` its dense nominal tables without weights.
inline void plan_gains_sampled(HostPlan& p, size_t B, size_t N, size_t M, size_t n_samples, const double*& X, const double*& U,
                               const double*& poly, const double*& xplan_fl, cilqr_obstacles& o, const double*& samp_off, double*& k_out,
                               double*& K_out, int32_t*& ok_out) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(poly, B * CILQR_POLY_COEFFS);
  p.in(xplan_fl, B * 2);
  o.weight = nullptr;
  plan_obstacles(p, M, o, B * M * N, 0);
  p.in(samp_off, B * M * n_samples * 3);
  p.out(k_out, B * 2 * N);
  p.out(K_out, B * 8 * N);
  p.out(ok_out, B);
}

// delta_sets: B, or 1 for one offset set shared by the solves.
inline void plan_rollout(HostPlan& p, size_t B, size_t N, size_t S, size_t delta_sets, const double*& X, const double*& U, const double*& k,
                         const double*& K, const double*& delta, double*& X_roll, double*& U_roll) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(k, B * 2 * N);
  p.in(K, B * 8 * N);
  p.in(delta, delta_sets * S * 4);
  p.out(X_roll, B * S * 4 * (N + 1));
  p.out(U_roll, B * S * 2 * N);
}

inline void plan_score_rollouts(HostPlan& p, size_t B, size_t N, size_t M, size_t S, const double*& X_roll, const double*& U_roll,
                                const double*& poly, const double*& xplan_fl, cilqr_obstacles& o, size_t span, size_t w_span,
                                double*& row_score, double*& risk, double*& total) {
  p.in(X_roll, B * S * 4 * (N + 1));
  p.in(U_roll, B * S * 2 * N);
  p.in(poly, B * CILQR_POLY_COEFFS);
  p.in(xplan_fl, B * 2);
  plan_obstacles(p, M, o, span, w_span);
  p.out(row_score, B * S * CILQR_SCORE_FIELDS);
  p.out(risk, B * CILQR_RISK_FIELDS);
  p.out(total, B);
}

// The kernel does not read obstacle weights: they do not travel.
inline void plan_rollout_risk(HostPlan& p, size_t B, size_t N, size_t M, size_t S, size_t delta_sets, const double*& X, const double*& U,
                              const double*& k, const double*& K, const double*& delta, cilqr_obstacles& o, size_t span, const double*& base,
                              double*& risk, int32_t*& step_hits, double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(k, B * 2 * N);
  p.in(K, B * 8 * N);
  p.in(delta, delta_sets * S * 4);
  o.weight = nullptr;
  plan_obstacles(p, M, o, span, 0);
  p.in(base, B);
  p.out(risk, B * CILQR_ROLLOUT_RISK_FIELDS);
  p.out(step_hits, B * N);
  p.out(total, B);
}

// cilqr_rollout_risk_sampled: M its n_obs, `o` its dense nominal tables without weights (12 arrays).
inline void plan_rollout_risk_sampled(HostPlan& p, size_t B, size_t N, size_t M, size_t n_samples, size_t S, size_t delta_sets,
                                      const double*& X, const double*& U, const double*& k, const double*& K, const double*& delta,
                                      cilqr_obstacles& o, const double*& samp_off, const double*& base, double*& risk,
                                      int32_t*& step_hits, double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(k, B * 2 * N);
  p.in(K, B * 8 * N);
  p.in(delta, delta_sets * S * 4);
  o.weight = nullptr;
  plan_obstacles(p, M, o, B * M * N, 0);
  p.in(samp_off, B * M * n_samples * 3);
  p.in(base, B);
  p.out(risk, B * CILQR_RRS_FIELDS);
  p.out(step_hits, B * N);
  p.out(total, B);
}

// cilqr_rollout_risk_map: no obstacle travels (the map is the handle's).  Per solve 17·N + 13 doubles and 4 per offset row: with
// B <= max_batch, N <= max_horizon and delta_sets·S <= max_batch·max_horizon that is at most 21·N + 13 of the 22·N + 34 doubles
// per unit of max_batch that host_arena_bytes reserves below, and the 10 arrays round up by less than its 32 x 16 bytes.
inline void plan_rollout_risk_map(HostPlan& p, size_t B, size_t N, size_t S, size_t delta_sets, const double*& X, const double*& U,
                                  const double*& k, const double*& K, const double*& delta, const double*& base, double*& risk,
                                  int32_t*& step_hits, int32_t*& unknown_hits, double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(k, B * 2 * N);
  p.in(K, B * 8 * N);
  p.in(delta, delta_sets * S * 4);
  p.in(base, B);
  p.out(risk, B * CILQR_MAP_RISK_FIELDS);
  p.out(step_hits, B * N);
  p.out(unknown_hits, B * N);
  p.out(total, B);
}

// cilqr_chance_risk: 13 arrays (cilqr_chance_risk_cov below declares one more, the most of any call); obstacle weights are not read and do not travel.  sigma_sets: B, or 1
// for one Σ0 shared by the solves.  Per solve 15·N + 6·M·N + 28 doubles without sigma_out and entry_p — inside the 22·N + 6·M·N +
// M + 34 per unit of max_batch that host_arena_bytes reserves below, for every B <= max_batch — and 31·N + 7·M·N + 44 with both,
// which fits for every B <= max_batch / 2; the shared W and the 13 roundings stay within its 32 x 16 bytes and that margin.
inline void plan_chance_risk(HostPlan& p, size_t B, size_t N, size_t M, size_t sigma_sets, const double*& X, const double*& U,
                             const double*& K, const double*& sigma0, const double*& W, cilqr_obstacles& o, size_t span,
                             const double*& base, double*& risk, double*& step_risk, double*& entry_p, double*& sigma_out,
                             double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(K, B * 8 * N);
  p.in(sigma0, sigma_sets * 16);
  p.in(W, 16);
  o.weight = nullptr;
  plan_obstacles(p, M, o, span, 0);
  p.in(base, B);
  p.out(risk, B * CILQR_CHANCE_FIELDS);
  p.out(step_risk, B * N);
  p.out(entry_p, B * M * N);
  p.out(sigma_out, B * (N + 1) * 16);
  p.out(total, B);
}

// cilqr_chance_risk_cov: the plan above with obs_cov, 3 doubles per entry of the span, behind the obstacles — 14 arrays.  With dense
// obstacles 15·N + 9·M·N + 28 doubles per solve without sigma_out and entry_p and 31·N + 10·M·N + 44 with both: half of either is
// inside what host_arena_bytes reserves below per unit of max_batch — the 22·N + 6·M·N + M + 34 of a solve, which the plans above
// quote, and the 6·N + 16 of a row beside it: 28·N + 6·M·N + M + 50 — so every B <= max_batch / 2 fits.
inline void plan_chance_risk_cov(HostPlan& p, size_t B, size_t N, size_t M, size_t sigma_sets, const double*& X, const double*& U,
                                 const double*& K, const double*& sigma0, const double*& W, cilqr_obstacles& o, size_t span,
                                 const double*& obs_cov, const double*& base, double*& risk, double*& step_risk, double*& entry_p,
                                 double*& sigma_out, double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(K, B * 8 * N);
  p.in(sigma0, sigma_sets * 16);
  p.in(W, 16);
  o.weight = nullptr;
  plan_obstacles(p, M, o, span, 0);
  p.in(obs_cov, span * 3);
  p.in(base, B);
  p.out(risk, B * CILQR_CHANCE_FIELDS);
  p.out(step_risk, B * N);
  p.out(entry_p, B * M * N);
  p.out(sigma_out, B * (N + 1) * 16);
  p.out(total, B);
}

// cilqr_predict_obstacles: 8 arrays.  Per track 24 doubles in (state, dimensions, covariance) and 6·N out for the table, 3·N more
// with cov_out and 16·N more with sigma_out; the shared noise is 16.  Against the same 28·N + 6·M·N + M + 50 per unit of max_batch
// (22·N + 6·M·N + M + 34 per solve and 6·N + 16 per row) that host_arena_bytes reserves below at the create sizes: T·M·(24 + 25·N) + 16 with every output fits for every T <= max_batch/8
// (M/8·(24 + 25·N) = 3·M + 3.125·M·N), T·M·(24 + 9·N) + 16 without sigma_out for every T <= max_batch/5 (4.8·M + 1.8·M·N); the 8
// roundings stay within its 32 x 16 bytes.
inline void plan_predict_obstacles(HostPlan& p, size_t T, size_t N, size_t M, const double*& track, const double*& track_dim,
                                   const double*& track_cov, const double*& noise, double*& pose_out, double*& dim_out,
                                   double*& cov_out, double*& sigma_out) {
  p.in(track, T * M * 6);
  p.in(track_dim, T * M * 2);
  p.in(track_cov, T * M * 16);
  p.in(noise, 16);
  p.out(pose_out, T * M * 4 * N);
  p.out(dim_out, T * M * 2 * N);
  p.out(cov_out, T * M * 3 * N);
  p.out(sigma_out, T * M * 16 * N);
}

// cilqr_track_update: 9 arrays at most.  In: the detections and their counts (`counts` int32: the span n_det_stride addresses, 0
// without n_det).  The state travels both ways as one array where state_in == state_out, as an input and an output otherwise; under
// CILQR_TRACK_RESET (`reset`) neither the incoming state nor the incoming world is read, so both are outputs only and state_in
// becomes the place of state_out.  Per world 32·M doubles of state (64·M with a separate state_out), 5·D + D/2 for the detections and
// assign, 9 for the world and 24·M for the three output tables: W·(88·M + 5.5·D + 9) at most, beside the counts.  With M <= the
// handle's max_obstacles and D <= 64 that is within the 28·N + 6·M·N + M + 50 per unit of max_batch that host_arena_bytes reserves
// below once max_horizon >= 15 (470 + 91·M against 361 + 88·M): every W <= max_batch fits there with one count per world, and the
// 9 roundings stay within its 32 x 16 bytes and that margin.
inline void plan_track_update(HostPlan& p, size_t W, size_t M, size_t D, size_t counts, bool reset, const double*& det,
                              const int32_t*& n_det, const double*& state_in, double*& state_out, double*& world, int32_t*& assign,
                              double*& track_out, double*& dim_out, double*& cov_out) {
  const bool in_place = !reset && state_in == state_out;
  p.in(det, W * D * 5);
  p.in(n_det, counts);
  if (!reset && !in_place) p.in(state_in, W * M * CILQR_TRACK_STATE);
  if (in_place) {
    p.inout(state_out, W * M * CILQR_TRACK_STATE);
    state_in = state_out;
  }
  if (!reset) p.inout(world, W * CILQR_TRACK_WORLD_FIELDS);
  if (!in_place) p.out(state_out, W * M * CILQR_TRACK_STATE);
  if (reset) {
    p.out(world, W * CILQR_TRACK_WORLD_FIELDS);
    state_in = state_out;
  }
  p.out(assign, W * D);
  p.out(track_out, W * M * 6);
  p.out(dim_out, W * M * 2);
  p.out(cov_out, W * M * 16);
}

// cilqr_tighten_obstacles: 8 arrays; obstacle weights are not read and do not travel; obs_cov travels as 3 doubles per entry of the
// span.  Per solve, with dense obstacles, 20·N + 15·M·N + 24 doubles with obs_cov and pose_out and 20·N + 8·M·N + 24 without them,
// against the 22·N + 6·M·N + M + 34 per unit of max_batch that host_arena_bytes reserves below: every B <= 2·max_batch/5 fits with
// both, every B <= 3·max_batch/4 without, and the 8 roundings stay within its 32 x 16 bytes.
inline void plan_tighten_obstacles(HostPlan& p, size_t B, size_t N, size_t M, const double*& X, const double*& sigma, cilqr_obstacles& o,
                                   size_t span, const double*& obs_cov, double*& pose_out, double*& dim_out, double*& tighten) {
  p.in(X, B * 4 * (N + 1));
  p.in(sigma, B * (N + 1) * 16);
  o.weight = nullptr;
  plan_obstacles(p, M, o, span, 0);
  p.in(obs_cov, span * 3);
  p.out(pose_out, B * M * 4 * N);
  p.out(dim_out, B * M * 2 * N);
  p.out(tighten, B * CILQR_TIGHTEN_FIELDS);
}

// cilqr_tighten_map: 4 arrays; the map is the handle's.  Per solve 20·N + 26 doubles — X, sigma, the tighten row — and one output
// layer of `cells` floats, cells/2 doubles: B·(20·N + 26 + cells/2) doubles against the max_batch·(22·max_horizon + 34) that
// host_arena_bytes reserves below; the 4 roundings stay within its 32 x 16 bytes.
inline void plan_tighten_map(HostPlan& p, size_t B, size_t N, size_t cells, const double*& X, const double*& sigma, float*& layer_out,
                             double*& tighten) {
  p.in(X, B * 4 * (N + 1));
  p.in(sigma, B * (N + 1) * 16);
  p.out(layer_out, B * cells);
  p.out(tighten, B * CILQR_TIGHTEN_MAP_FIELDS);
}

// cilqr_rasterize_tracks: 6 arrays; the map is the handle's; obstacle weights are not read and do not travel; obs_cov travels as 3
// doubles per entry of the span.  Per solve 4·N + 10 doubles — X, the fields row — and one output layer of `cells` floats, cells/2
// doubles; the tracks are 9 doubles per entry of the span, M·N entries for one shared set: B·(4·N + 10 + cells/2) + 9·span doubles
// against the 28·N + 6·M·N + M + 50 per unit of max_batch that host_arena_bytes reserves below at create sizes that admit the call.
// On the node's 150 x 100 map at N = 50 with one shared set of 8 tracks every B <= max_batch/8 fits once max_batch >= 8; the 6
// roundings stay within its 32 x 16 bytes.
inline void plan_rasterize_tracks(HostPlan& p, size_t B, size_t N, size_t cells, const double*& X, cilqr_obstacles& o, size_t span,
                                  const double*& obs_cov, float*& layer_out, double*& fields) {
  p.in(X, B * 4 * (N + 1));
  o.weight = nullptr;
  plan_obstacles(p, 1, o, span, 0);
  p.in(obs_cov, span * 3);
  p.out(layer_out, B * cells);
  p.out(fields, B * CILQR_TRACK_MAP_FIELDS);
}

// cilqr_chance_risk_map: 10 arrays; the map is the handle's and no gain travels.  Per solve 20·N + 30 doubles — X, sigma, base, the
// risk row, total — and 3·N more with the three per-step outputs; the Q nodes and weights, shared by the batch, are 4·Q doubles.
// Against the 22·N + 34 per unit of max_batch that host_arena_bytes reserves below: without per-step outputs every B <= max_batch
// fits once 4·Q <= max_batch·(2·max_horizon + 4), with them every B <= 7·max_batch/8 once 4·Q <= max_batch·(max_horizon + 7); the
// 10 roundings stay within its 32 x 16 bytes.
inline void plan_chance_risk_map(HostPlan& p, size_t B, size_t N, size_t Q, const double*& X, const double*& sigma, const double*& nodes,
                                 const double*& weights, const double*& base, double*& risk, double*& step_risk, double*& step_occ,
                                 double*& step_unknown, double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(sigma, B * (N + 1) * 16);
  p.in(nodes, Q * 3);
  p.in(weights, Q);
  p.in(base, B);
  p.out(risk, B * CILQR_CHANCE_MAP_FIELDS);
  p.out(step_risk, B * N);
  p.out(step_occ, B * N);
  p.out(step_unknown, B * N);
  p.out(total, B);
}

// cilqr_chance_risk_sampled: 11 arrays; M its n_obs, the nominal tables dense; no gain and no weight travels.  With E = M·n_samples
// (<= max_obstacles) and M <= E/2, per solve 20·N + 6·M·N + 3·E + 30 doubles — X, sigma, the nominal tables, the offsets, base, the
// risk row, total — plus N + M·N with step_risk and pair_p and E·N with entry_p: at most 21·N + 3.5·E·N + 3·E + 30 without entry_p
// and 21·N + 4.5·E·N + 3·E + 30 with it, against the 22·N + 6·E·N + E + 34 per unit of max_batch that host_arena_bytes reserves
// below at the create sizes.  Without entry_p every B <= max_batch fits; with it every B <= max_batch fits on a handle of
// max_horizon >= 2 and every B <= max_batch/2 on one of max_horizon 1; the 11 roundings stay within its 32 x 16 bytes.
inline void plan_chance_sampled(HostPlan& p, size_t B, size_t N, size_t M, size_t n_samples, const double*& X, const double*& sigma,
                                const double*& nom_pose, const double*& nom_dim, const double*& samp_off, const double*& base,
                                double*& risk, double*& step_risk, double*& pair_p, double*& entry_p, double*& total) {
  p.in(X, B * 4 * (N + 1));
  p.in(sigma, B * (N + 1) * 16);
  p.in(nom_pose, B * M * N * 4);
  p.in(nom_dim, B * M * N * 2);
  p.in(samp_off, B * M * n_samples * 3);
  p.in(base, B);
  p.out(risk, B * CILQR_CRS_FIELDS);
  p.out(step_risk, B * N);
  p.out(pair_p, B * M * N);
  p.out(entry_p, B * M * n_samples * N);
  p.out(total, B);
}

// cilqr_footprint_check: 8 arrays; R = B·S rows; obstacle weights are not read and do not travel.  Per row 5.5·N + 18 doubles with
// every output — X, base, the fp row, step_clearance, step_occ (N floats), total — and the obstacles are 6 doubles per entry of the
// span: R·(6·N + 18) + 6·span at most, against the 28·N + 6·M·N + M + 50 per unit of max_batch that host_arena_bytes reserves below:
// every R <= max_batch fits with a span within the B·M·N of dense tables, and the 8 roundings stay within its 32 x 16 bytes.
inline void plan_footprint(HostPlan& p, size_t R, size_t N, size_t M, const double*& X, cilqr_obstacles& o, size_t span, const double*& base,
                           double*& fp, double*& step_clearance, float*& step_occ, double*& total) {
  p.in(X, R * 4 * (N + 1));
  o.weight = nullptr;
  plan_obstacles(p, M, o, span, 0);
  p.in(base, R);
  p.out(fp, R * CILQR_FOOTPRINT_FIELDS);
  p.out(step_clearance, R * N);
  p.out(step_occ, R * N);
  p.out(total, R);
}

// cilqr_map_distance: 3 arrays of 4 bytes a cell: the layers' span in, d2_out and dist_out out.  The arena is sized by the solves,
// not by maps: the call fits where (span + 2·L·cells)/2 doubles do — the node's 150 x 100 map with both outputs takes 22 500 doubles
// a layer against the 28·N + 6·M·N + M + 50 per unit of max_batch that host_arena_bytes reserves below — and returns the transport's
// error where it does not.
inline void plan_map_distance(HostPlan& p, size_t L, size_t cells, size_t span, const float*& layer, int32_t*& d2_out, float*& dist_out) {
  p.in(layer, span);
  p.out(d2_out, L * cells);
  p.out(dist_out, L * cells);
}

// cilqr_inflate_map: 3 arrays of 4 bytes a cell: the layers' span and d2 in, layer_out out; fits as plan_map_distance does.
inline void plan_inflate_map(HostPlan& p, size_t L, size_t cells, size_t span, const float*& layer, const int32_t*& d2, float*& layer_out) {
  p.in(layer, span);
  p.in(d2, L * cells);
  p.out(layer_out, L * cells);
}

// cilqr_map_obstacles: 9 arrays.  In: d2 and the poses; then `work`, scratch that travels neither way (a place and no host
// address); out: label_out, n_out, comp and the three optional tables.  Three arrays of 4 bytes a cell and 24 doubles a row; fits
// as plan_map_distance does.
inline void plan_map_obstacles(HostPlan& p, size_t L, size_t cells, size_t K, size_t poses, const int32_t*& d2, const double*& pose,
                               int32_t*& work, int32_t*& label_out, int32_t*& n_out, double*& comp, double*& boxes, double*& pose_out,
                               double*& dim_out) {
  p.in(d2, L * cells);
  p.in(pose, poses * 3);
  work = nullptr;
  p.out(work, L * cells, true);
  p.out(label_out, L * cells);
  p.out(n_out, L * 4);
  p.out(comp, L * K * CILQR_MAP_OBSTACLE_FIELDS);
  p.out(boxes, L * K * 5);
  p.out(pose_out, L * K * 4);
  p.out(dim_out, L * K * 2);
}

// cilqr_clear_movers: 8 arrays at most.  In: the layers' span, label, comp and the mover form (assign and M state rows a layer, or
// mask); out: layer_out, owner_out and the fields rows.  Four arrays of 4 bytes a cell, 13 doubles and one or two int32 a row, 32·M
// doubles a layer in the tracker form, 8 doubles a layer of fields; fits as plan_map_distance does.
inline void plan_clear_movers(HostPlan& p, size_t L, size_t cells, size_t span, size_t K, size_t M, const float*& layer,
                              const int32_t*& label, const double*& comp, const int32_t*& assign, const double*& state,
                              const int32_t*& mask, float*& layer_out, int32_t*& owner_out, double*& fields) {
  p.in(layer, span);
  p.in(label, L * cells);
  p.in(comp, L * K * CILQR_MAP_OBSTACLE_FIELDS);
  p.in(assign, L * K);
  p.in(state, L * M * CILQR_TRACK_STATE);
  p.in(mask, L * K);
  p.out(layer_out, L * cells);
  p.out(owner_out, L * cells);
  p.out(fields, L * CILQR_CLEAR_MOVERS_FIELDS);
}

// cilqr_map_clearance: 5 arrays; R = B·S rows; the map is the handle's.  Per row 5·N + 14 doubles with every output — X, base, the mc
// row, step_clearance, total — against the 28·N + 50 per unit of max_batch that host_arena_bytes reserves below: every R <= max_batch
// fits, and the 5 roundings stay within its 32 x 16 bytes.
inline void plan_map_clearance(HostPlan& p, size_t R, size_t N, const double*& X, const double*& base, double*& mc, double*& step_clearance,
                               double*& total) {
  p.in(X, R * 4 * (N + 1));
  p.in(base, R);
  p.out(mc, R * CILQR_MAP_CLEARANCE_FIELDS);
  p.out(step_clearance, R * N);
  p.out(total, R);
}

// cilqr_stop_plans: 8 arrays; B plans, R = B·D rows.  In: X, U, the D levels, plan_cost; out: X_stop, U_stop, the sp row, cost.  With
// B <= R and D <= R that is R·(12·N + 19) doubles at most, against the 22·N + 34 per unit of max_batch that host_arena_bytes reserves
// below: every R <= max_batch fits, and the 8 roundings stay within its 32 x 16 bytes.
inline void plan_stop_plans(HostPlan& p, size_t B, size_t N, size_t D, const double*& X, const double*& U, const double*& decel,
                            const double*& plan_cost, double*& X_stop, double*& U_stop, double*& sp, double*& cost) {
  const size_t R = B * D;
  p.in(X, B * 4 * (N + 1));
  p.in(U, B * 2 * N);
  p.in(decel, D);
  p.in(plan_cost, B);
  p.out(X_stop, R * 4 * (N + 1));
  p.out(U_stop, R * 2 * N);
  p.out(sp, R * CILQR_STOP_FIELDS);
  p.out(cost, R);
}

// Bytes of the arena cilqr_create reserves for a handle of max_batch B, max_horizon N, max_obstacles M.  What include/cilqr.h
// promises about "the buffers reserved at create" is a statement about this number: it does not change.
inline size_t host_arena_bytes(size_t B, size_t N, size_t M) {
  // The solve and score forms: their own plans at the create sizes with dense obstacle tables — B·M·N entries with B·M weights,
  // or with B·M sample-offset records in place of the weights (n_obs·n_samples <= M).  Serves "the span the strides address
  // must fit the B·M·N reserved at create" of cilqr_solve_batch_obstacles and cilqr_score_batch.
  static double host;  // (a non-null host pointer to declare with; never read)
  size_t cap = 0;
  // (`sampled`, 0 or 1, is passed as n_samples: B·M·1 records of 3 doubles are the B·M sample-offset records)
  for (size_t sampled = 0; sampled < 2; ++sampled) {
    for (int score = 0; score < 2; ++score) {
      cilqr_obstacles o = {&host, &host, sampled ? nullptr : &host, 0, 0, 0, 0};
      const double *a = &host, *b = &host, *c = &host, *d = &host, *off = &host;
      double *u = &host, *x = &host, *j = &host;
      int32_t *it = nullptr, *st = nullptr;
      HostPlan p(nullptr);
      if (score) plan_score(p, B, N, M, sampled, a, b, c, d, o, B * M * N, sampled ? 0 : B * M, off, x, j);
      else plan_solve(p, B, N, M, sampled, a, u, c, d, o, B * M * N, sampled ? 0 : B * M, off, x, j, it, st);
      if (p.end > cap) cap = p.end;
    }
  }
  // The gains / rollout / rollout-score / rollout-risk forms, per unit of max_batch in doubles:
  //   one SOLVE's arrays — path, obstacle weights and entries, nominal X and U, gains k and K, risk + total + ok — serving
  //   "B <= max_batch", and
  //   one ROW's arrays — a rollout's X and U, its 4 offsets, its score row — serving "host-buffer form: B*S <= max_batch";
  //   cilqr_rollout_risk moves no rows, which leaves the row share to its offsets: 4 doubles each for up to
  //   max_batch·max_horizon of them, "(delta_batch_stride ? B : 1)*S <= max_batch*max_horizon always fits";
  //   and 32 roundings to 16 bytes.
  const size_t per_solve = (CILQR_POLY_COEFFS + 2) + (M + 6 * M * N) + (4 * (N + 1) + 2 * N) + (2 * N + 8 * N) + (CILQR_RISK_FIELDS + 1 + 1);
  const size_t per_row = (4 * (N + 1) + 2 * N) + 4 + CILQR_SCORE_FIELDS;
  const size_t risk = B * (per_solve + per_row) * sizeof(double) + 32 * 16;
  return risk > cap ? risk : cap;
}

}  // namespace cilqr
