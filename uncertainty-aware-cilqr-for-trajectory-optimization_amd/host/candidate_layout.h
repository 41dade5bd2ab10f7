// candidate_layout.h — which stages a run of iLQR::run_candidates (run_step under a tightening) enqueues, and where their arrays lie
// in the one device block the facade keeps.  No HIP, no library: tests/cpp/candidate_layout_dump.cpp and tests/test_candidate_layout.py
// check it without a GPU.  The setters size the block and the run picks its stages from the SAME CandidateModes, so a stage cannot
// run on arrays that were sized 0.
#pragma once

#include <stddef.h>

#include "cilqr.h"

namespace cilqr_host {

struct CandidateModes {
  // what the setters put in force
  bool noise = false;          // set_pose_noise_check(_fused): offsets are set
  bool fused = false;          // ... and the fused setter was the last of the two (it stays when the offsets are emptied)
  bool cov = false;            // set_pose_covariance_check
  bool scov = false;           // set_sample_covariance_check
  bool sampled = false;        // set_obstacle_samples
  bool cov_judge = false;      // set_obstacle_covariance_check
  bool cmap = false;           // set_map_covariance_check
  bool map = false;            // set_map_risk_check
  bool tighten = false;        // set_chance_tightening
  bool map_tighten = false;    // set_map_tightening
  bool track_map = false;      // set_track_map with rounds > 0
  bool min_total = false;      // set_candidate_pick(MinTotalCost)
  bool footprint = false;      // set_footprint_check
  bool map_clearance = false;  // set_map_clearance_check
  bool stop_fallback = false;  // set_stop_fallback
  // the scene at the time of the run: no setter reserves by these, so the layout never reads them
  bool map_set = false;        // an uncertainty map is set
  bool obstacles = false;      // M > 0
  bool tracks = false;         // set_tracked_obstacles is in force

  // ---- what the layout is sized by -------------------------------------------------------------------------------------------
  // no stored rollout rows; the nominal score rows, their totals, the step counts and the map risk check's outputs instead
  bool fused_form() const { return fused || cov || !noise; }
  bool chance_inputs() const { return cov || scov; }              // Sigma0, W and the chance rows
  bool cmap_arrays() const { return chance_inputs() && cmap; }    // the nodes and the map covariance check's outputs
  bool sigma_kept() const { return cmap_arrays() || scov; }       // every Sigma_t of the chance call
  bool chain() const { return tighten || map_tighten; }           // the rounds' gains and covariance chain
  bool block_used() const { return noise || cov || scov || chain() || track_map || footprint || map_clearance; }  // a setter that is on keeps the block reserved

  // ---- which stages a run enqueues --------------------------------------------------------------------------------------------
  bool track_rounds() const { return track_map && tracks && map_set; }
  bool in_block() const { return noise || cov || scov || tighten || map_tighten || track_rounds() || footprint || map_clearance_check(); }  // else: the host-buffer forms
  bool plain() const { return !noise && !cov && !scov; }  // no check behind the solve: the pick of run_candidates itself
  bool sampled_solve() const { return sampled; }
  bool obstacle_rounds() const { return tighten && obstacles; }
  bool map_rounds() const { return map_tighten && map_set; }
  bool rounds() const { return obstacle_rounds() || map_rounds() || track_rounds(); }
  bool fused_check() const { return noise && fused; }
  bool scored() const { return scov || fused_check() || (!noise && min_total); }  // last_scores is filled
  bool score_before_gains() const { return !noise && !scov; }
  bool gains() const { return !plain(); }
  bool stored_rows_risk() const { return noise && !fused; }
  bool fused_risk() const { return fused_check() && !sampled; }
  bool fused_sampled_risk() const { return fused_check() && sampled; }
  bool chance() const { return cov || scov; }  // (scov: with M = 0, for its Sigma_t and the steps that are not finite)
  bool chance_sampled() const { return scov; }
  bool map_covariance() const { return cmap && map_set && chance(); }
  bool map_rollout_risk() const { return map && map_set && (fused_check() || cov); }
  bool footprint_check() const { return footprint; }  // the last check but one in front of the pick, whatever else is in force
  bool map_clearance_check() const { return map_clearance && map_set; }  // behind it: the last stage in front of the pick, while a map is set
  bool stop_fallback_check() const { return stop_fallback && footprint; }  // behind the pick: stop plans, their checks and a second pick
};

struct CandidateSizes {
  size_t B = 1;          // max_candidates
  size_t N = 0;          // horizon
  size_t M = 0;          // max_obstacles
  size_t S = 0;          // pose-noise offsets
  size_t n_obs = 0;      // nominal obstacles under set_obstacle_samples
  size_t n_samples = 0;  // ... and samples of each
  size_t Q = 0;          // quadrature nodes of set_map_covariance_check
  size_t D = 0;          // braking levels of set_stop_fallback
  // rollouts per candidate: the covariance check has no draws and keeps ONE zero offset, the plan itself, for the map risk call
  size_t rollouts(const CandidateModes& m) const { return m.cov ? 1 : S; }
};

// Every array of the block, in the order it is laid out.
#define CILQR_CANDIDATE_ARRAYS(F)                                                                                                  \
  F(x0) F(U) F(poly) F(fl) F(pose) F(dim) F(soff) F(X) F(J) F(iters) F(status) F(k) F(K) F(ok) F(delta) F(Xr) F(Ur) F(rows) F(risk) \
  F(total) F(pair) F(score) F(base) F(hits) F(mrisk) F(mtotal) F(mhits) F(munk) F(s0) F(W) F(crisk) F(cstep) F(ccov) F(csig) F(qn)  \
  F(qw) F(cmrisk) F(cmstep) F(cmtotal) F(ts0) F(tW) F(tsig) F(trisk) F(tpose) F(tdim) F(tg) F(tcov) F(tmg) F(tkcov) F(tkf) F(srisk) \
  F(stotal) F(mcrow) F(mcstep) F(mctotal) F(fprow) F(fpstep) F(fptotal)

// The stop fallback's arrays, behind every array above: the levels, the stop rows (at most B of them: floor(B / D) candidates at D
// levels), their sp rows and costs, the S = D footprint check's rows and totals, the map clearance check's, the second pick.
#define CILQR_CANDIDATE_STOP_ARRAYS(F) F(stlv) F(stX) F(stU) F(stsp) F(stcost) F(stfp) F(stfptotal) F(stmc) F(stmctotal) F(stpair)

struct CandidateLayout {  // offsets in doubles (from candidate_layout) or sizes in doubles (from candidate_sizes)
#define F(name) size_t name = 0;
  CILQR_CANDIDATE_ARRAYS(F)
  CILQR_CANDIDATE_STOP_ARRAYS(F)
#undef F
  size_t end = 0;
};

// What each array holds, in doubles; int32 arrays (iters, status, ok, the step counts) share double slots.
inline CandidateLayout candidate_sizes(const CandidateModes& m, const CandidateSizes& z) {
  const size_t B = z.B, N = z.N, M = z.M, S = z.rollouts(m), ff = m.fused_form(), R = ff ? 0 : B * S, steps = (B * N + 1) / 2;
  const size_t ci = m.chance_inputs(), cm = m.cmap_arrays(), chain = m.chain(), tg = m.tighten, trk = m.track_map;
  CandidateLayout s;
  s.x0 = B * 4; s.U = B * 2 * N; s.poly = B * CILQR_POLY_COEFFS; s.fl = B * 2;
  // with obstacle samples: per-candidate nominal tables and offsets in place of the one shared set (n_obs * n_samples <= M)
  s.pose = m.sampled ? B * z.n_obs * 4 * N : M * 4 * N; s.dim = m.sampled ? B * z.n_obs * 2 * N : M * 2 * N;
  s.soff = m.sampled ? B * z.n_obs * z.n_samples * 3 : 0;
  s.X = B * 4 * (N + 1); s.J = B; s.iters = B; s.status = B;
  s.k = B * 2 * N; s.K = B * 8 * N; s.ok = B;
  s.delta = S * 4;
  s.Xr = R * 4 * (N + 1); s.Ur = R * 2 * N; s.rows = R * CILQR_SCORE_FIELDS;
  s.risk = B * (m.sampled ? CILQR_RRS_FIELDS : ff ? CILQR_ROLLOUT_RISK_FIELDS : CILQR_RISK_FIELDS); s.total = B; s.pair = 2;
  s.score = ff * B * CILQR_SCORE_FIELDS; s.base = ff * B; s.hits = ff * steps;
  // the map risk check's outputs (a few doubles per candidate: reserved with the fused form whether or not the check is on)
  s.mrisk = ff * B * CILQR_MAP_RISK_FIELDS; s.mtotal = ff * B; s.mhits = ff * steps; s.munk = ff * steps;
  // the chance call's inputs and outputs; the obstacles' covariance for its judge (set_obstacle_covariance_check)
  s.s0 = ci * 16; s.W = ci * 16; s.crisk = ci * B * CILQR_CHANCE_FIELDS; s.cstep = m.cov ? B * N : 0;
  s.ccov = m.cov && m.cov_judge ? M * N * 3 : 0;
  // the map covariance check: every Sigma_t of the chance call, the nodes and weights, its outputs
  s.csig = m.sigma_kept() ? B * (N + 1) * 16 : 0; s.qn = cm * z.Q * 3; s.qw = cm * z.Q;
  s.cmrisk = cm * B * CILQR_CHANCE_MAP_FIELDS; s.cmstep = m.cov && m.cmap ? B * N : 0; s.cmtotal = cm * B;
  // the rounds: Sigma0, W, every Sigma_t, the risk row of the round's input plan, the inflated dense table, the fields, obs_cov
  // (the map tightening shares the chain's arrays and adds its fields; its layers are floats and lie outside this block)
  s.ts0 = chain * 16; s.tW = chain * 16; s.tsig = chain * B * (N + 1) * 16; s.trisk = chain * B * CILQR_CHANCE_FIELDS;
  s.tpose = tg * B * M * 4 * N; s.tdim = tg * B * M * 2 * N; s.tg = tg * B * CILQR_TIGHTEN_FIELDS; s.tcov = tg * M * N * 3;
  s.tmg = m.map_tighten ? B * CILQR_TIGHTEN_MAP_FIELDS : 0;
  // the track map's rounds: the tracks' covariance by the packed obstacles' strides, the fields
  s.tkcov = trk * M * N * 3; s.tkf = trk * B * CILQR_TRACK_MAP_FIELDS;
  // the sample covariance check's rows and total
  s.srisk = m.scov ? B * CILQR_CRS_FIELDS : 0; s.stotal = m.scov ? B : 0;
  // the map clearance check's rows, its per-step clearances and its total: empty with the flag off, so that every offset is what it was
  // (in FRONT of the footprint check's, which tests/test_footprint.py pins as the last three)
  s.mcrow = m.map_clearance ? B * CILQR_MAP_CLEARANCE_FIELDS : 0; s.mcstep = m.map_clearance ? B * N : 0; s.mctotal = m.map_clearance ? B : 0;
  // the footprint check's rows, its per-step clearances and its total: at the END, so that every earlier offset is what it was
  s.fprow = m.footprint ? B * CILQR_FOOTPRINT_FIELDS : 0; s.fpstep = m.footprint ? B * N : 0; s.fptotal = m.footprint ? B : 0;
  // the stop fallback: empty with the flag off, so that every offset and `end` are what they were
  const size_t st = m.stop_fallback;
  s.stlv = st * z.D; s.stX = st * B * 4 * (N + 1); s.stU = st * B * 2 * N; s.stsp = st * B * CILQR_STOP_FIELDS; s.stcost = st * B;
  s.stfp = st * B * CILQR_FOOTPRINT_FIELDS; s.stfptotal = st * B; s.stmc = st * B * CILQR_MAP_CLEARANCE_FIELDS; s.stmctotal = st * B;
  s.stpair = st * 2;
  return s;
}

// The offsets: the arrays one behind the other, each starting on an even double so that int32 views stay aligned.
inline CandidateLayout candidate_layout(const CandidateModes& m, const CandidateSizes& z) {
  const CandidateLayout s = candidate_sizes(m, z);
  CandidateLayout L;
  size_t o = 0;
#define F(name) L.name = o; o += (s.name + 1) & ~(size_t)1;
  CILQR_CANDIDATE_ARRAYS(F)
  CILQR_CANDIDATE_STOP_ARRAYS(F)
#undef F
  L.end = o;
  return L;
}

}  // namespace cilqr_host
