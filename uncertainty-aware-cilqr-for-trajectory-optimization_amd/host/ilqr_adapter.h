// ilqr_adapter.h — host-side C++ mirror of the reference planner façade, above the C-ABI of include/cilqr.h.
//
// The reference's ROS node drives a stateful `iLQR` object (I/iLQR.h:16-59; I/ = CILQR/src/ilqr/include/ilqr/):
//     ilqrplanner.set_global_plan(global_path);  ilqrplanner.set_Obstacle(obstacles);
//     ilqrplanner.run_step(ego_state);           → X_result, U_result, ref_traj_result
// (I/ilqr_uncertainty_node.cpp:113-130).  This class keeps those names, argument meanings and the persistent, un-shifted
// warm start (`control_seq`, I/iLQR.cpp:9-15,253) so that call sequence is unchanged; every solve goes through
// cilqr_solve_batch_obstacles with B = 1 (or B = candidates, see run_candidates) on the HIP device.  There is no CPU path.
//
// Differences from the reference interface, all forced by the boundary:
//   * Eigen types are replaced by the column-major `Matrix` below (Eigen is not a dependency of this library);
//   * device/HIP failures throw std::runtime_error (the reference solver cannot fail that way);
//   * the reference's Uncertainty class is not in its repository: the `Uncertainty` below carries what its
//     constructor is given at the call site (I/ilqr_uncertainty_node.cpp:111-112) and the cost is the one include/cilqr.h
//     defines at cilqr_set_uncertainty_map (parity unpinned); set_uncertainty_map / clear_uncertainty_map keep the
//     reference's names and effect (I/iLQR.cpp:28-35);
//   * nothing is printed to stdout (the reference prints three lines per solve, I/iLQR.cpp:240-242); the same facts are
//     available as last_iterations / last_exit / last_cost.
#pragma once

#include <vector>

#include "candidate_layout.h"
#include "cilqr.h"

namespace cilqr_host {

// Dense column-major matrix of doubles: element (r, c) at a[r + rows*c] — Eigen::MatrixXd's default layout.
struct Matrix {
  int rows = 0, cols = 0;
  std::vector<double> a;
  Matrix() = default;
  Matrix(int r, int c) : rows(r), cols(c), a((size_t)r * c, 0.0) {}
  double& operator()(int r, int c) { return a[(size_t)c * rows + r]; }
  double operator()(int r, int c) const { return a[(size_t)c * rows + r]; }
};

using Parameters = cilqr_params;  // POD mirror of the reference's class Parameters (I/Parameters.h)
Parameters default_parameters();  // Parameters::Parameters(), I/Parameters.cpp:3-75

// Obstacle(Parameters p, MatrixXd dimension /*2×N*/, MatrixXd relative_pos_array /*4×N*/), I/Obstacle.h:13-25.
class Obstacle {
 public:
  Obstacle(const Parameters& p, const Matrix& dimension, const Matrix& relative_pos_array)
      : p(p), dimension(dimension), relative_pos_array(relative_pos_array) {}
  Parameters p;
  Matrix dimension;           // 2 × horizon: (length, width) per step
  Matrix relative_pos_array;  // 4 × horizon: (x, y, v, theta) per step
};

// What the reference node builds its Uncertainty object from, every tick (I/ilqr_uncertainty_node.cpp:111-112): the blurred
// occupancy layer of the map node (grid_map_msg "uncertainty_map"; rows×cols float32 column-major, 0..100, NaN unknown), its
// vehicle-frame geometry centred at (x_center, y_center) (map_param), and the vehicle pose the map was made at
// (map_msg.info.origin).  probes: footprint sampling of the safe_length × safe_width rectangle (include/cilqr.h).
struct Uncertainty {
  std::vector<float> layer;
  cilqr_map_geom geom{};
  double pose_x = 0.0, pose_y = 0.0, pose_theta = 0.0;
  int probes_l = 3, probes_w = 3;
};

// vehiclepub/Experiment as the node fills it (I/ilqr_uncertainty_node.cpp:243-284): start_pos[4], X flattened column by
// column (4 per step, horizon + 1 steps), U likewise (2 per step), planning_time in seconds.  (Its ros::Time start_time
// belongs to the caller.)  Column-major flattening is the memory order of X_result / U_result, so these are copies.
struct Experiment {
  double planning_time = 0.0;
  std::vector<double> start_pos, X, U;
};
Experiment flatten_experiment(const double start_pos[4], double planning_time, const Matrix& X, const Matrix& U);

// What run_candidates ranks the solved candidates by.  MinTrackingCost: J = Constraints::get_J, tracking and control effort only
// (the default).  MinTotalCost: the `total` column of cilqr_score_batch — J plus the control-barrier, obstacle-barrier and
// uncertainty-map costs, NaN (never picked) for a candidate whose collision share exceeds max_collision.
enum class CandidatePick { MinTrackingCost, MinTotalCost };

class iLQR {
 public:
  // max_candidates > 1 reserves device buffers for run_candidates().
  explicit iLQR(const Parameters& params, int device = 0, int max_obstacles = 64, int max_candidates = 1);
  ~iLQR();
  iLQR(const iLQR&) = delete;
  iLQR& operator=(const iLQR&) = delete;

  void set_Obstacle(const std::vector<Obstacle>& obstacles);  // I/iLQR.cpp:20-23 (deep copy, like the reference)
  void clear_Obstacle();                                      // :24-27
  void set_uncertainty_map(const Uncertainty& uncertainty);    // :28-31 → Constraints::set_uncertainty_map (I/Constraints.cpp:520-524)
  void clear_uncertainty_map();                               // :32-35
  void set_global_plan(const Matrix& global_plan);            // :41-45, 2 × P waypoints

  // I/iLQR.cpp:201-245.  U is the warm start on entry and U_result on return; x_local_plan is the local plan's x row
  // (only its first and last entries are read, I/Constraints.cpp:31-33).
  void get_optimal_control_seq(const double x_0[4], Matrix& U, const double poly_coeffs[6],
                               const std::vector<double>& x_local_plan);
  void run_step(const double ego_state[4]);  // :247-255

  // Batched form of run_step for sampled ego states (e.g. the node's Gaussian pose noise, I/ilqr_uncertainty_node.cpp:82-110):
  // solves every candidate from the current warm start in ONE launch, keeps the minimum-cost one (cilqr_argmin_device)
  // as X_result/U_result/control_seq and returns its index.  The obstacle set travels once for all candidates
  // (cilqr_solve_batch_obstacles, batch stride 0).
  // With set_candidate_pick(CandidatePick::MinTotalCost, max_collision) the solved batch is scored on the device against the same
  // shared obstacle set (cilqr_score_batch, batch stride 0) and the pick is the strict-< first minimum of `total`, a NaN never
  // winning (the convention of cilqr_argmin_device): the cheapest among the safe.  last_scores then holds the B × 8 score rows
  // (cilqr_score_field).  If every candidate is rejected the call returns -1 and X_result, U_result, the warm start and the
  // last_* fields stay as they were.  max_collision = 0 rejects any contact, 1 rejects nothing on collision grounds.
  int run_candidates(const std::vector<double>& ego_states /* 4 per candidate */);
  void set_candidate_pick(CandidatePick pick, double max_collision = 0.0);
  // Pose-noise check.  The node plans from a pose it knows to be wrong: it adds Gaussian noise to the ego pose before run_step.
  // `offsets` are S draws of that noise, (dx, dy, dv, dtheta) each, made ONCE by the node with its own sigmas.  With a non-empty set,
  // run_candidates judges every solved candidate by where the vehicle may really be: solve -> cilqr_gains_batch_device(lamb) ->
  // cilqr_rollout_batch_device (k_scale 0: the plan is tracked by the feedback gains from each offset start) ->
  // cilqr_score_rollouts_device(max_risk) -> cilqr_argmin_device on its `total`, one after the other on one stream with nothing but
  // the pick, the risk rows and the picked candidate's results coming back.  last_risk then holds CILQR_RISK_FIELDS per candidate.
  // The pick is the cheapest mean total among the candidates whose share of colliding rollouts is at most max_risk; when every
  // candidate is rejected the call returns -1 and X_result, U_result, the warm start and the last_* result fields stay as they were
  // (the contract of set_candidate_pick, which this check takes precedence over; last_scores is then empty).  lamb: the
  // regularisation of the gains' backward pass (1.0: the reference's starting value).  Device buffers are sized here, from
  // max_candidates x offsets / 4 and the current horizon, not per call.  An empty `offsets` switches the check off (the default).
  void set_pose_noise_check(const std::vector<double>& offsets, double max_risk, double lamb = 1.0);
  // The same check without stored rollouts: solve -> cilqr_gains_batch_device(lamb) -> cilqr_score_batch_device (the nominal
  // `total` of every candidate, max_collision 1: nothing is rejected there) -> cilqr_rollout_risk_device(k_scale 0, max_risk, base =
  // those totals) -> cilqr_argmin_device on its `total`.  The pick is the cheapest NOMINAL total among the candidates whose share of
  // colliding rollouts is at most max_risk (the stored-rows check ranks by the mean total over the rollouts).  last_risk then holds
  // CILQR_ROLLOUT_RISK_FIELDS per candidate (cilqr_rollout_risk_field), last_step_hits the rollouts that hit at each step, horizon
  // per candidate, last_scores the nominal score rows.  Rejection, the -1 return and an empty `offsets` as above.  More than 256
  // offsets take ceil(S/256) partial records per candidate of the max_candidates the handle holds: run_candidates then takes at most
  // max_candidates / ceil(S/256) candidates.  Whichever of the two setters was called last applies.
  void set_pose_noise_check_fused(const std::vector<double>& offsets, double max_risk, double lamb = 1.0);
  // Map risk check: the fused check above looks at the obstacles of set_Obstacle only, and in the node that channel is switched off —
  // the blurred costmap of set_uncertainty_map is all the planner knows of obstacles (I/ilqr_uncertainty_node.cpp:111-113, 151-189).
  // It has effect under set_pose_noise_check_fused while an uncertainty map is set: run_candidates then enqueues, on the check's
  // stream, ... -> cilqr_rollout_risk(_sampled)_device (its `total`) -> cilqr_rollout_risk_map_device(k_scale 0, occ_threshold,
  // max_risk, base = that total) -> cilqr_argmin_device on the map call's `total`.  A candidate is then also rejected when the share
  // of its rollouts whose footprint probes enter cells above occ_threshold exceeds max_risk (unknown_hits: a probe outside the map
  // or on a cell that is not finite counts as entering one).  last_map_risk holds CILQR_MAP_RISK_FIELDS per candidate
  // (cilqr_map_risk_field), last_map_step_hits and last_map_unknown_hits the rollouts that hit / are unknown at each step, horizon
  // per candidate.  With no map set, or under any other pick, behaviour is what it is without this call and the three fields are
  // empty.  An occ_threshold that is NaN switches the check off (the default).
  void set_map_risk_check(double occ_threshold, double max_risk, bool unknown_hits = false);
  // Footprint check: the last gate in front of the pick.  Every check above judges a plan by the solver's surrogates (an ego circle's
  // centre inside an inflated ellipse; probes on safe_length x safe_width); this one asks whether the vehicle's length x width
  // rectangle, grown by `margin`, touches an obstacle's rectangle or covers a map cell above occ_threshold
  // (cilqr_footprint_check_device).  run_candidates then enqueues it as the LAST stage in front of cilqr_argmin_device, on the final
  // plan, against the ORIGINAL obstacles and the original map, whatever else is in force: its base is the total before it, or J where
  // no check ran, and a candidate with an obstacle hit, a clearance below min_clearance or a map hit is rejected (its total is NaN;
  // -1 when all are).  It needs no other setter: alone it is a valid configuration (solve -> (score under MinTotalCost) -> footprint
  // -> pick).  occ_threshold = +infinity leaves the map out of the decision; unknown_hits: a covered cell outside the map or NaN
  // rejects.  last_footprint holds CILQR_FOOTPRINT_FIELDS per candidate (cilqr_footprint_field), last_footprint_clearance the
  // smallest clearance per step, horizon per candidate.  With set_obstacle_samples the run throws std::logic_error (the check has no
  // sampled form).  on = false switches it off (the default).
  void set_footprint_check(double min_clearance, double occ_threshold, double margin = 0.0, bool unknown_hits = false, bool on = true);
  // Map clearance check: the map half of min_clearance.  The footprint check measures distance to obstacle rectangles only; against
  // the map it knows overlap alone.  This check asks how far the vehicle's rectangle, grown by `margin`, stays from the nearest
  // occupied cell (value > occ_threshold; unknown_seeds: NaN cells too) within `reach` metres (cilqr_map_clearance_device).  It runs
  // while a map is set: run_candidates enqueues it as the LAST stage in front of cilqr_argmin_device, behind the footprint check when
  // both are on, on the final plan against the ORIGINAL map; its base is the total before it, or J where no check ran, and a
  // candidate that comes closer than min_clearance, or has a step that is not finite, is rejected (its total is NaN; -1 when all
  // are).  It needs no other setter.  last_map_clearance holds CILQR_MAP_CLEARANCE_FIELDS per candidate (cilqr_map_clearance_field),
  // last_map_step_clearance the clearance per step, horizon per candidate; both are empty when no map was set.  on = false switches
  // it off (the default).
  void set_map_clearance_check(double min_clearance, double reach, double occ_threshold, double margin = 0.0, bool unknown_seeds = false,
                               bool on = true);
  // Stop fallback: a plan for the tick on which every candidate is rejected.  While it is on run_candidates enqueues, behind its normal
  // pipeline and pick, on the same stream with nothing coming back in between: cilqr_stop_plans_device on the B final plans (D =
  // decels.size() braking levels, gentlest first by convention, plan_cost = J, decel_weight 1e6) -> cilqr_footprint_check_device with
  // S = D on the stop rows, against the ORIGINAL obstacles and map, with the margin, min_clearance and threshold of set_footprint_check
  // -> cilqr_map_clearance_device with S = D when that check is on and a map is set -> a second cilqr_argmin_device over the B*D
  // totals.  It is always enqueued: the fallback costs a fixed latency per tick, not a second round trip on the tick that needs it.
  // Where the normal pick is >= 0 the return value, X_result, U_result, the warm start and every other last_* field are bit for bit
  // what they are without this setter, and last_stop_level is -1.  Where it is -1 and a stop row is clear, the call returns that row's
  // candidate, X_result / U_result are the stop row, last_stop_level is its level index, and the warm start stays as it was (a stop
  // plan is not a solve); where no stop row is clear either the call returns -1.  last_stop holds CILQR_STOP_FIELDS per row
  // (row = candidate * D + level), last_stop_footprint CILQR_FOOTPRINT_FIELDS per row, last_stop_pick the second pick's row or -1.
  // It needs set_footprint_check: without it run_candidates throws std::logic_error (a stop row nobody judged is no fallback), and
  // with set_obstacle_samples it throws as the footprint check does.  The handle holds max_candidates rows: under the fallback
  // run_candidates takes at most floor(max_candidates / D) candidates and throws std::runtime_error beyond.  on = false switches it
  // off (the default).
  void set_stop_fallback(const std::vector<double>& decels, int hold = 1, double max_deviation = 0.5, bool on = true);
  // Pose-covariance check: the analytic counterpart of the fused pose-noise check.  Instead of S draws of the pose noise the node
  // hands over its covariance: Sigma0, 4 x 4 column-major over (x, y, v, theta) (only row <= column is read), and the process noise
  // W added per step (nullable: none).  run_candidates then enqueues, on the check's stream: solve -> (under MinTotalCost
  // cilqr_score_batch_device, max_collision 1: the nominal totals) -> cilqr_gains_batch_device(lamb) -> cilqr_chance_risk_device
  // (max_risk; base = those totals, or J under MinTrackingCost) -> cilqr_argmin_device on its `total`.  A candidate is rejected when
  // CR_STEP_RISK — with sum_bound CR_SUM_RISK — exceeds max_risk: the largest per-step (the summed) Gaussian chance that an ego circle
  // enters an obstacle of set_Obstacle under the closed-loop covariance along its plan.  No samples, no seed, and it orders candidates
  // the sampled check calls 0 / S.  last_chance_risk holds CILQR_CHANCE_FIELDS per candidate (cilqr_chance_risk_field),
  // last_step_risk the per-step bound r_t, horizon per candidate; last_scores the nominal score rows under MinTotalCost.  Rejection
  // and the -1 return as under set_pose_noise_check.  set_map_risk_check composes after it through `base` while an uncertainty map
  // is set: with no draws to roll out, the map call sees ONE rollout per candidate, from the zero offset — the plan itself — so a
  // plan whose own footprint enters cells above occ_threshold is rejected whenever max_risk of set_map_risk_check is below 1.
  // set_map_covariance_check composes after it the same way and is the check that uses the covariance against the map; with both
  // map checks set the chain is chance -> map covariance -> map rollout, each taking the total before it as its base.
  // Together with set_pose_noise_check(_fused) offsets, or with set_obstacle_samples (the sampled scene form has a setter of its own:
  // set_sample_covariance_check), the setters throw std::logic_error naming the conflict.  Sigma0 == nullptr switches the check off
  // (the default).
  void set_pose_covariance_check(const double Sigma0[16], const double* W, double max_risk, double lamb = 1.0, bool sum_bound = false);
  // Map covariance check: the analytic counterpart of set_map_risk_check.  It has effect under set_pose_covariance_check while an
  // uncertainty map is set: run_candidates then enqueues, on the check's stream, solve -> (score) -> cilqr_gains_batch_device ->
  // cilqr_chance_risk_device (its `total` and every Sigma_t in sigma_out; with no obstacle set, the live node's case, it runs with
  // M = 0 for its Sigma_t alone and rejects nothing) -> cilqr_chance_risk_map_device(occ_threshold, max_risk, base = that total) ->
  // cilqr_argmin_device on the map call's `total`.  The nodes, the nx x ny x nth tensor product of Gauss-Hermite rules of
  // cilqr_pose_quadrature (1 ... 9 per axis), are built here, once.  A candidate is rejected when CM_STEP_RISK — with sum_bound
  // CM_SUM_RISK — exceeds max_risk: the largest per-step (the summed) weighted mass of node poses whose footprint probes enter cells
  // above occ_threshold (unknown_hits: a probe outside the map or on a cell that is not finite counts as entering one).
  // last_chance_map_risk holds CILQR_CHANCE_MAP_FIELDS per candidate (cilqr_chance_map_field), last_map_step_risk the per-step r_t,
  // horizon per candidate.  With no map set, or without the covariance check, behaviour is what it is without this call and both
  // fields are empty.  An occ_threshold that is NaN switches the check off (the default).
  void set_map_covariance_check(double occ_threshold, double max_risk, int nx = 5, int ny = 5, int nth = 3, bool sum_bound = false,
                                bool unknown_hits = false);
  // Chance-constraint tightening: every check above judges a solved plan and can only reject it; this feeds the pose covariance back
  // into the solve.  Sigma0 and W as in set_pose_covariance_check; eps the chance allowed per obstacle entry (kappa =
  // cilqr_chance_kappa(eps) standard deviations).  While set, run_step (get_optimal_control_seq) and run_candidates follow their solve
  // by `rounds` rounds, enqueued on the check's stream with nothing coming back in between:
  //   cilqr_gains_batch_device(lamb), on the obstacles of set_Obstacle -> cilqr_chance_risk_device (its sigma_out) ->
  //   cilqr_tighten_obstacles_device(kappa, max_inflate: no semi-axis grows by more) -> cilqr_solve_batch_obstacles_device on the
  //   inflated table, warm-started from the U the solve before it left.
  // X_result, U_result, the warm start, last_cost, last_iterations and last_exit are the LAST re-solve's.  Every score or risk check
  // that follows — set_candidate_pick, set_pose_noise_check(_fused), set_pose_covariance_check, set_map_risk_check — judges that final
  // plan against the ORIGINAL obstacles.  last_tighten holds CILQR_TIGHTEN_FIELDS per solve (cilqr_tighten_field) of the last round,
  // last_tighten_risk_before the CR_STEP_RISK of the plan that round started from, one per solve; with no obstacle set there is
  // nothing to inflate, the rounds are skipped and both stay empty.  The barriers are soft and the tightening is a first-order,
  // axis-wise one (include/cilqr.h): it moves a plan that has room to move and guarantees nothing — keep a check behind it.
  // Sigma0 == nullptr or rounds == 0 switches it off (the default).  Together with set_obstacle_samples (whichever comes second)
  // the setters throw std::logic_error: the sampled solve has no inflated form here.
  void set_chance_tightening(const double Sigma0[16], const double* W, double eps, int rounds = 1, double max_inflate = 2.0, double lamb = 1.0);
  // The obstacles' own position covariance for the tightening (obs_cov of cilqr_tighten_obstacles): (xx, xy, yy) in the world frame
  // per obstacle of set_Obstacle, in its order — 3 * M values, constant over the horizon, or 3 * M * horizon, obstacle-major.  Empty:
  // none (the default).  A size that matches neither makes the next run throw std::runtime_error.
  void set_obstacle_covariance(const std::vector<double>& cov);
  // Tracked obstacles: what a tracker hands over once per tick in place of a finished table.  tracks holds 6 values per vehicle,
  // (x, y, v, theta, a, omega); dims 2, (length, width); cov 16, P_0 column-major over (x, y, v, theta) (only row <= column is read),
  // or empty: none; Q 16 values added per step, or empty: none.  The vehicles are predicted over params.horizon by
  // cilqr_predict_obstacles (the host form; see include/cilqr.h for the model) and the result is installed where set_Obstacle and
  // set_obstacle_covariance (its 3 * M * horizon form) would put it: every later call behaves as if those two had been called with
  // the predicted table and (xx, xy, yy) of every P_t.  When params.horizon has changed by the next run the vehicles are predicted
  // again.  clear_Obstacle removes the tracks, the obstacles and that covariance; set_Obstacle replaces the obstacles and removes the
  // covariance the prediction installed.  A size that does not match throws std::runtime_error.
  void set_tracked_obstacles(const std::vector<double>& tracks, const std::vector<double>& dims, const std::vector<double>& cov,
                             const std::vector<double>& Q);
  // Off (the default): nothing changes.  On: the judge of set_pose_covariance_check is cilqr_chance_risk_cov_device with whatever
  // obstacle covariance is set (set_obstacle_covariance, set_tracked_obstacles); with none set it is cilqr_chance_risk_device as
  // before.  Under set_chance_tightening the final plan is then judged against the ORIGINAL obstacles WITH their covariance — what
  // the tightening inflated them by.  A covariance whose size matches neither form makes the next run throw std::runtime_error.
  void set_obstacle_covariance_check(bool on);
  // Map tightening: the map counterpart of set_chance_tightening, for the configuration the live node runs — no obstacle set, the
  // blurred costmap of set_uncertainty_map the planner's only obstacle information — where every check above can only reject.  Sigma0,
  // W, eps, rounds and lamb as in set_chance_tightening.  While it and an uncertainty map are set, run_step (get_optimal_control_seq)
  // and run_candidates follow their solve by `rounds` rounds, enqueued on the checks' stream with nothing coming back in between:
  //   cilqr_gains_batch_device(lamb) -> cilqr_chance_risk_device, for its sigma_out (with M = 0 when no obstacle is set) ->
  //   cilqr_tighten_map_device(kappa = cilqr_chance_kappa(eps), max_inflate: no cell reaches further, in metres) on the ORIGINAL
  //   layer, so inflation never compounds over rounds -> the tightened per-solve layers set on the handle -> the re-solve,
  //   warm-started from the U the solve before it left -> the original map set on the handle again.
  // After the rounds the original map is on the handle, bit for bit, and every later score or risk check — set_candidate_pick,
  // set_map_risk_check, set_map_covariance_check, ... — judges the final plan against it.  last_tighten_map holds
  // CILQR_TIGHTEN_MAP_FIELDS per solve (cilqr_tighten_map_field) of the last round, last_tighten_map_risk_before the CR_STEP_RISK of
  // the plan that round started from, one per solve: the chance of contact with the OBSTACLES of set_Obstacle, 0 with none set (the
  // map has no part in it).  With no map set the rounds are skipped and both stay empty.  When set_chance_tightening is also set and
  // obstacles are set, one round tightens both and re-solves once; the two setters must then agree on Sigma0, W, lamb and rounds, or
  // the second one throws std::logic_error (switching either off leaves the other's inputs as they are).  The layer is soft, first order and axis-capped
  // (include/cilqr.h): it guarantees nothing — keep a check behind it.  While it is on, the layer of set_uncertainty_map lives in
  // device memory of this object, beside one tightened layer per candidate, and the handle reads it there.
  // Sigma0 == nullptr or rounds == 0 switches it off (the default: nothing changes for existing callers).  Together with
  // set_obstacle_samples (whichever comes second) the setters throw std::logic_error, like set_chance_tightening.
  void set_map_tightening(const double Sigma0[16], const double* W, double eps, int rounds = 1, double max_inflate = 1.0, double lamb = 1.0);
  // Track map: the tracks of set_tracked_obstacles rasterised into the map along each plan, for the configuration the live node runs.
  // While it is on, tracks are set (set_tracked_obstacles) and an uncertainty map is set, run_step (get_optimal_control_seq) and
  // run_candidates follow their solve by `rounds` rounds, enqueued on the checks' stream with nothing coming back in between:
  //   cilqr_rasterize_tracks_device(inflate, z_max, window) along the current plans, always from the ORIGINAL layer, with the
  //   predicted covariance -> the per-solve layers set on the handle (layer_stride = rows*cols) -> the re-solve, warm-started from
  //   the U the solve before it left -> the original map set on the handle again.
  // ellipses = false: the SOLVES run with M = 0, so the tracks reach the planner through the map only — the live node's
  // configuration; every later score and check (set_candidate_pick, set_pose_covariance_check with set_obstacle_covariance_check,
  // the pose-noise checks, the map checks) still sees the tracks, and judges the final plan against them and the original map.
  // With set_map_tightening on, one round is: gains and covariance chain -> rasterise -> cilqr_tighten_map_device on the RASTERISED
  // layers -> one re-solve; with set_chance_tightening the inflated ellipses go into that same re-solve.  The round counts must then
  // agree, and set_chance_tightening beside ellipses = false has nothing to inflate: a run throws std::logic_error for either.
  // last_track_map holds CILQR_TRACK_MAP_FIELDS per solve (cilqr_track_map_field) of the last round; with no tracks or no map set the
  // rounds are skipped and it stays empty.  The layer is soft and first order (include/cilqr.h): it guarantees nothing — keep a check
  // behind it.  While rounds > 0 the layer of set_uncertainty_map lives in device memory of this object, as under set_map_tightening,
  // beside one layer per candidate (two with set_map_tightening).  With obstacle samples (set_obstacle_samples,
  // set_sample_covariance_check) in force a run under it throws std::logic_error, like set_map_tightening.
  // rounds == 0 switches it off (the default: nothing changes for existing callers).  A negative rounds or window, or an inflate or
  // z_max that is negative or not finite, throws std::runtime_error.
  void set_track_map(double inflate, double z_max, int window, int rounds = 1, bool ellipses = true);
  // Map obstacles: the other direction of the map channel.  In the live node's configuration the occupied cells of the layer are all
  // the planner knows of obstacles, and the barrier, CILQR_FP_CLEARANCE and the chance risk have no rectangle to act on.  While this
  // setter is on, every set_uncertainty_map runs, on that layer and pose, cilqr_map_distance_device(occ_threshold) ->
  // cilqr_map_obstacles_device(gap2 = floor((gap/res)^2), 8-connectivity, min_cells, max_size, pad, K) and installs the rows written BEHIND
  // the obstacles of set_Obstacle, constant over the horizon: the solve, and every later score and check, sees them as if set_Obstacle
  // had been given them too.  last_map_obstacles holds the rows, 5 values each — (x, y, yaw, size_x, size_y), the boxes of
  // cilqr_map_obstacles — and last_map_obstacle_counts its n_out.  set_Obstacle and clear_Obstacle replace the obstacles in front of
  // the rows and keep the rows; clear_uncertainty_map, or on = false, removes them.  The rows count against max_obstacles
  // (std::runtime_error beyond).  The two calls run in a device block of this object's own — a map's arrays, three of 4 bytes a cell,
  // do not fit the arena of a handle made for a few candidates — grown when a larger map or K comes, never per call; their results are
  // those of the host forms, bit for bit.  With
  // set_obstacle_samples, set_tracked_obstacles or set_obstacle_covariance in force a run throws std::logic_error: the rows have
  // neither samples nor a covariance.  Off (the default): nothing changes for existing callers.
  void set_map_obstacles(double occ_threshold, double gap, int min_cells, double max_size, double pad, int K, bool on = true);
  // Map tracker: the rows of set_map_obstacles followed across ticks, so that a moving vehicle reaches the solver with a velocity and
  // a covariance and not as a box that stands where it is now.  It needs set_map_obstacles (std::logic_error without it) with
  // K <= CILQR_TRACK_MAX_DETECTIONS, and 1 <= slots <= min(CILQR_TRACK_MAX_SLOTS, max_obstacles) (std::runtime_error otherwise, and for
  // a filter cilqr_track_update rejects).  While it is on, every set_uncertainty_map runs cilqr_map_distance_device ->
  // cilqr_map_obstacles_device -> cilqr_track_update_device(f, slots; the counts read where cilqr_map_obstacles left them), the first
  // map after switching on or after clear_Obstacle with CILQR_TRACK_RESET.  The CONFIRMED rows are installed through the path of
  // set_tracked_obstacles — predicted over params.horizon with their covariance, in slot order — and the static rows of
  // set_map_obstacles are not appended: the judges that read tracks (set_obstacle_covariance_check, set_chance_tightening with the
  // obstacles' covariance, set_track_map) have their input in the map-only configuration.  The tracker is the one producer of
  // tracks: set_tracked_obstacles, set_Obstacle and set_obstacle_covariance beside it throw std::logic_error, and so does switching it
  // on while tracks of set_tracked_obstacles are set.  last_tracks holds 8 values per confirmed row — (id, x, y, v, theta, length,
  // width, slot) — and last_track_counts the world record (cilqr_track_world_field).  on = false removes the tracks and, with a map
  // set, puts the static rows back.  Off (the default): nothing changes for existing callers.
  void set_map_tracker(const cilqr_track_filter& f, int slots, bool on = true);
  // Mover clearing: the static layer.  Under set_map_tracker a vehicle confirmed as moving reaches the planner twice: as a track, which
  // predicts it away, and as a blob of occupied cells that stands where it is now for the whole horizon; in the map-only configuration
  // the blob wins.  It needs set_map_tracker (std::logic_error without it; the tracker cannot be switched off under it).  While it is
  // on, every set_uncertainty_map runs cilqr_map_distance_device -> cilqr_map_obstacles_device -> cilqr_track_update_device on the layer
  // AS GIVEN and then, in this object's own device block behind them, cilqr_clear_movers_device in its tracker form: the filter's
  // min_hits, v_clear in m/s, halo2 = floor((halo/res)^2) cells^2 with halo in metres, evaluated in double as written — 0.3 / 0.1 is just below 3 there, so give a halo a little
  // above the radius meant, 0.31 for three cells of 0.1 m — (std::runtime_error for a v_clear, halo or fill
  // the call rejects, at the setter or, where the limit depends on the map's resolution, at the map), `fill` for the cleared cells.
  // The CLEARED layer is then the map: it is set on the handle and is the "original" every later stage starts from and judges
  // against — the solve, the rounds of set_map_tightening and set_track_map, set_map_risk_check, set_map_covariance_check, the map
  // half of set_footprint_check and set_map_clearance_check.  A cleared vehicle is gone from the map: it comes back through its
  // track only, so keep a judge that reads tracks behind it (set_footprint_check, set_obstacle_covariance_check, set_track_map).
  // last_mover_clearing holds the CILQR_CLEAR_MOVERS_FIELDS of the last map (cilqr_clear_movers_field).  on = false, or
  // clear_uncertainty_map, puts things back: with a map set the layer as given is the map again.  Off (the default): nothing changes
  // for existing callers.
  void set_mover_clearing(double v_clear, double halo, float fill = 0.0f, bool on = true);
  // Test hook: cilqr_debug_uncertainty_cost on the map this object's handle holds right now, at n = states.size() / 4 states
  // (x, y, v, theta) -> n costs, then 2n of vx, then 3n of mx.  Throws std::runtime_error when no map is set.
  std::vector<double> debug_map_cost(const std::vector<double>& states) const;

  // Sampled obstacles: the uncertainty-aware scene form.  `offsets` holds n_obs x n_samples x 3 doubles, (dx, dy, dtheta) per pose
  // sample, drawn ONCE by the node with its own sigmas; the obstacles of set_Obstacle are then the NOMINAL ones (n_obs of them, in
  // the same order, n_obs * n_samples <= max_obstacles), and every sample weighs params.w_obstacle / n_samples.  With a non-empty
  // set, run_step and run_candidates solve with cilqr_solve_batch_sampled(_device), MinTotalCost scores with
  // cilqr_score_batch_sampled (its collision share is the largest share of an obstacle's samples hit at one step), and under
  // set_pose_noise_check_fused run_candidates runs, on one stream: cilqr_solve_batch_sampled_device ->
  // cilqr_gains_batch_sampled_device(lamb) -> cilqr_score_batch_sampled_device (nominal totals, max_collision 1) ->
  // cilqr_rollout_risk_sampled_device(k_scale 0, max_risk, base = those totals) -> cilqr_argmin_device.  last_risk then holds
  // CILQR_RRS_FIELDS per candidate (cilqr_rollout_risk_sampled_field): a candidate is rejected when the mean over the ego-pose draws
  // of its worst sample share exceeds max_risk.  The stored-rows check has no sampled form: with samples set,
  // set_pose_noise_check (and a run_candidates under it) throws std::logic_error naming set_pose_noise_check_fused.  An empty
  // `offsets` switches the samples off (the default): everything behaves as without this call.
  void set_obstacle_samples(const std::vector<double>& offsets, int n_samples);
  // Sample covariance check: set_pose_covariance_check for the sampled scene form.  Sigma0, W, lamb and sum_bound as there.  It has
  // effect while set_obstacle_samples is in force; without samples set run_candidates throws std::logic_error naming
  // set_pose_covariance_check.  Together with set_pose_noise_check(_fused) offsets, whichever comes second throws std::logic_error:
  // the pose noise is given either as a covariance or as draws.  run_candidates then enqueues, on the checks' stream:
  // cilqr_solve_batch_sampled_device -> cilqr_gains_batch_sampled_device(lamb) -> cilqr_score_batch_sampled_device (nominal totals,
  // max_collision 1) -> cilqr_chance_risk_device (M = 0: every Sigma_t in sigma_out; base = those totals, so a step whose U_t or K_t
  // is not finite is marked in its total) -> cilqr_chance_risk_sampled_device (base = that total) -> cilqr_chance_risk_map_device
  // (base = that total; only while set_map_covariance_check is on and an uncertainty map is set) -> cilqr_argmin_device.  A
  // candidate is rejected when CRS_STEP_RISK — with sum_bound CRS_SUM_RISK — exceeds max_risk: the largest per-step (the summed)
  // chance of contact, under the closed-loop covariance along its plan, with the obstacles' empirical pose distributions.
  // last_chance_risk_sampled holds CILQR_CRS_FIELDS per candidate (cilqr_chance_risk_sampled_field), last_scores the nominal score
  // rows, last_chance_map_risk the map call's rows when it ran.  Rejection and the -1 return as under set_pose_noise_check.
  // Sigma0 == nullptr switches the check off (the default).
  void set_sample_covariance_check(const double Sigma0[16], const double* W, double max_risk, double lamb = 1.0, bool sum_bound = false);

  Parameters params;
  Matrix X_result;         // 4 × (horizon + 1)
  Matrix U_result;         // 2 × horizon
  Matrix ref_traj_result;  // 2 × n_local_wpts
  int last_iterations = 0;
  int last_exit = 0;  // cilqr_exit
  double last_cost = 0.0;
  std::vector<double> last_scores;  // run_candidates under MinTotalCost: CILQR_SCORE_FIELDS per candidate; empty otherwise
  std::vector<double> last_risk;  // run_candidates under set_pose_noise_check: CILQR_RISK_FIELDS per candidate; empty otherwise
                                  // (under set_pose_noise_check_fused: CILQR_ROLLOUT_RISK_FIELDS per candidate, CILQR_RRS_FIELDS with
                                  // obstacle samples set)
  std::vector<int32_t> last_step_hits;  // run_candidates under set_pose_noise_check_fused: horizon per candidate; empty otherwise
  // run_candidates with the map risk check in effect (set_map_risk_check); empty otherwise
  std::vector<double> last_map_risk;               // CILQR_MAP_RISK_FIELDS per candidate
  std::vector<int32_t> last_map_step_hits, last_map_unknown_hits;  // horizon per candidate
  // run_candidates under set_footprint_check; empty otherwise
  std::vector<double> last_footprint, last_footprint_clearance;  // CILQR_FOOTPRINT_FIELDS per candidate; horizon per candidate
  // run_candidates under set_map_clearance_check with a map set; empty otherwise
  std::vector<double> last_map_clearance, last_map_step_clearance;  // CILQR_MAP_CLEARANCE_FIELDS per candidate; horizon per candidate
  // run_candidates under set_stop_fallback; empty otherwise (last_stop_level: -1 whenever the published plan is a solved one)
  std::vector<double> last_stop, last_stop_footprint;  // CILQR_STOP_FIELDS / CILQR_FOOTPRINT_FIELDS per row = candidate * D + level
  int last_stop_pick = -1, last_stop_level = -1;

  // Path-aligned planning frame (include/cilqr.h, "path-aligned planning frame").  While on, run_step and run_candidates on the
  // unchecked path run: framed pre-step (cilqr_local_plan_frames) -> the obstacle rows into the frames (cilqr_frame_obstacles) ->
  // the map pose into the frames while a map is set (cilqr_frame_poses) -> the unchanged solve, and the score under MinTotalCost ->
  // X out of the frame (cilqr_frame_states).  X_result and ref_traj_result are in the map frame, as they are without the setter;
  // U_result and the warm start are frame-free.  global_inflation: CILQR_FRAME_GLOBAL_INFLATION for moving obstacles.  Off, the
  // default, every path is bit for bit what it is without this setter.  The stages that run in the device block
  // (CandidateModes::in_block(): noise, covariance and sampled checks, the tightenings, the track map, footprint, map clearance, stop
  // fallback), the tightened run_step and obstacle samples are not framed yet: with one of them and this setter both on, run_step /
  // run_candidates throw std::logic_error naming set_path_frame.
  void set_path_frame(bool on, bool global_inflation = false);
  std::vector<double> last_frames;        // [B][CILQR_FRAME_DOUBLES] of the last framed call (B = 1 after run_step); empty when off
  std::vector<int32_t> last_frame_info;   // [B] CILQR_FRAME_* bits
  // run_candidates under set_pose_covariance_check; empty otherwise
  std::vector<double> last_chance_risk, last_step_risk;  // CILQR_CHANCE_FIELDS per candidate; horizon per candidate
  // run_candidates with the map covariance check in effect (set_map_covariance_check); empty otherwise
  std::vector<double> last_chance_map_risk, last_map_step_risk;  // CILQR_CHANCE_MAP_FIELDS per candidate; horizon per candidate
  // run_candidates under set_sample_covariance_check; empty otherwise
  std::vector<double> last_chance_risk_sampled;  // CILQR_CRS_FIELDS per candidate
  // run_step / run_candidates under set_chance_tightening with obstacles set; empty otherwise
  std::vector<double> last_tighten, last_tighten_risk_before;  // CILQR_TIGHTEN_FIELDS per solve; CR_STEP_RISK per solve
  // run_step / run_candidates under set_map_tightening with an uncertainty map set; empty otherwise
  std::vector<double> last_tighten_map, last_tighten_map_risk_before;  // CILQR_TIGHTEN_MAP_FIELDS per solve; CR_STEP_RISK per solve
  // run_step / run_candidates under set_track_map with tracks and an uncertainty map set; empty otherwise
  std::vector<double> last_track_map;  // CILQR_TRACK_MAP_FIELDS per solve
  // set_uncertainty_map under set_map_obstacles; empty / zero otherwise
  std::vector<double> last_map_obstacles;  // 5 per row: (x, y, yaw, size_x, size_y)
  int32_t last_map_obstacle_counts[4] = {0, 0, 0, 0};  // n_out of cilqr_map_obstacles
  // set_uncertainty_map under set_map_tracker; empty / zero otherwise
  std::vector<double> last_tracks;  // 8 per confirmed row: (id, x, y, v, theta, length, width, slot)
  double last_track_counts[CILQR_TRACK_WORLD_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // the world record of cilqr_track_update
  // set_uncertainty_map under set_mover_clearing; zero otherwise
  double last_mover_clearing[CILQR_CLEAR_MOVERS_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};  // the fields of cilqr_clear_movers

 private:
  void pack_obstacles();
  cilqr_obstacles obstacle_strides();  // the packed set, shared by every solve of a call (batch stride 0)
  cilqr_handle* h_ = nullptr;
  int device_, max_obstacles_, max_candidates_;
  CandidatePick pick_ = CandidatePick::MinTrackingCost;
  double max_collision_ = 0.0;
  Matrix control_seq_;  // I/iLQR.h:34
  Matrix global_plan_;
  std::vector<Obstacle> obstacles_;
  // set_Obstacle: every obstacle's columns are bit-identical over the horizon (how the reference node feeds static obstacles,
  // I/ilqr_uncertainty_node.cpp:175-185): then one column per obstacle is packed and passed with step stride 0
  bool held_ = false;
  int packed_horizon_ = -1;  // the horizon obs_pose_ / obs_dim_ were packed for
  std::vector<double> obs_pose_, obs_dim_;  // packed ONCE: [obstacle][4N] / [2N], or [obstacle][4] / [2] when held_
  // tracked obstacles (set_tracked_obstacles): the inputs as given, and the horizon they were last predicted over (-1: none set)
  std::vector<double> tracks_, track_dims_, track_cov_, track_Q_;
  int tracked_horizon_ = -1;
  void install_tracked();  // predicts over params.horizon and fills obstacles_, obs_cov_ and the packed forms
  bool obs_cov_check_ = false;  // set_obstacle_covariance_check
  // obstacle samples (set_obstacle_samples): the offsets [n_obs][n_samples][3]; n_samples_ == 0: none
  std::vector<double> samples_;
  int n_samples_ = 0;
  // the compact form for B solves sharing the obstacle set: dense nominal tables [B][n_obs][4N] / [2N], offsets [B][n_obs][n_samples][3];
  // returns n_obs
  int pack_sampled(int B, std::vector<double>& pose, std::vector<double>& dim, std::vector<double>& off) const;
  double sample_weight() const { return params.w_obstacle / n_samples_; }
  // The checks' pipeline ("The facade's candidate pipeline"): every run_candidates but the unchecked one, and run_step under
  // a tightening, runs in ONE device block on a stream of its own.  candidate_layout.h says, from modes() and sizes(), where the
  // block's arrays lie and which stages a run enqueues; Block (the pointer, the stream, up / down) is opaque here so that this header
  // needs no HIP.
  struct Block;
  struct Candidates;  // what the prologue makes: the local plans and the replicated warm start
  struct Solved;      // one solve's X, U, J, iterations and exit
  CandidateModes modes() const;
  CandidateSizes sizes() const;
  Block block() const;
  void reserve_block();  // lays the block out for modes() and sizes(), allocates it and uploads what the setters fixed
  void reserve_block_if_used() { if (modes().block_used()) reserve_block(); }
  Candidates plan_candidates(int B, const std::vector<double>& ego_states);
  int run_candidates_in_block(int B, const std::vector<double>& ego_states, const CandidateModes& m);
  cilqr_obstacles upload_obstacles(const Block& d);  // the packed set into the block: the same strides over the device copies
  void fetch_solved(const Block& d, int b, Solved& s) const;  // enqueues
  void install(const Solved& s, Matrix& U);                  // after the wait: X_result, U (the warm start) and U_result, last_*
  void clear_round_fields();      // last_tighten*, last_track_map
  void clear_candidate_fields();  // every last_* vector run_candidates owns
  CandidateLayout layout_{};
  int block_horizon_ = -1;  // the horizon the block was laid out for
  void* block_dev_ = nullptr;
  void* block_stream_ = nullptr;
  // Sigma0, W, the bound and lamb of a covariance setter; Sigma0 and W travel with every call (32 doubles)
  struct CovarianceParams {
    bool on = false, has_W = false, sum = false;
    double sigma0[16] = {}, W[16] = {}, max_risk = 1.0, lamb = 1.0;
    void set(const double* Sigma0, const double* W_, double max_risk_, double lamb_, bool sum_);
    bool same_inputs(const double* Sigma0, const double* W_, double lamb_) const;
  };
  const double* upload(const Block& d, const CovarianceParams& p, size_t s0_at, size_t W_at) const;  // returns W in the block, or null
  CovarianceParams cov_, scov_;  // set_pose_covariance_check, set_sample_covariance_check
  CovarianceParams tg_;          // the one set both tightenings read (on, sum and max_risk unused)
  // pose-noise check: the offsets as given
  bool noise_fused_ = false;  // set_pose_noise_check_fused was the last setter
  void set_noise(const std::vector<double>& offsets, double max_risk, double lamb, bool fused);
  std::vector<double> noise_;
  double max_risk_ = 1.0, noise_lamb_ = 1.0;
  // map risk check: in effect when map_check_ (set_map_risk_check), map_set_ (an uncertainty map is set) and a fused or covariance check
  bool map_check_ = false, map_set_ = false, map_unknown_hits_ = false;
  double map_threshold_ = 0.0, map_max_risk_ = 1.0;
  // footprint check (set_footprint_check)
  bool fp_check_ = false, fp_unknown_hits_ = false;
  double fp_min_clearance_ = 0.0, fp_threshold_ = 0.0, fp_margin_ = 0.0;
  // stop fallback (set_stop_fallback)
  bool stop_on_ = false;
  bool frame_on_ = false, frame_global_inflation_ = false;
  void* frame_dev_ = nullptr;   // while a map is set under set_path_frame: the layer and one framed pose per candidate
  size_t frame_dev_cap_ = 0;    // bytes
  int run_framed(int B, const std::vector<double>& ego_states, bool step);  // run_step (B = 1, step) and the unchecked run_candidates
  std::vector<double> stop_decel_;
  int stop_hold_ = 1;
  double stop_max_deviation_ = 0.5;
  // map clearance check (set_map_clearance_check)
  bool mc_check_ = false, mc_unknown_seeds_ = false;
  double mc_min_clearance_ = 0.0, mc_reach_ = 0.0, mc_threshold_ = 0.0, mc_margin_ = 0.0;
  // map covariance check: in effect when cmap_check_ (set_map_covariance_check), map_set_ and a covariance check; the nodes as built
  bool cmap_check_ = false, cmap_sum_ = false, cmap_unknown_hits_ = false;
  double cmap_threshold_ = 0.0, cmap_max_risk_ = 1.0;
  std::vector<double> cmap_nodes_, cmap_weights_;
  // chance-constraint tightening (set_chance_tightening, set_obstacle_covariance)
  bool tighten_ = false;
  int tg_rounds_ = 0;
  double tg_kappa_ = 0.0, tg_cap_ = 2.0;
  std::vector<double> obs_cov_, obs_cov_packed_;  // as given; and addressed by the packed obstacles' strides, 3 per entry
  // `rounds` rounds behind a solve of B plans in the block (x0, U, poly, fl, X, J, iters, status in place); returns a C-ABI code
  int tighten_rounds(const Block& d, int B, const cilqr_obstacles* po);
  void fetch_tighten(const Block& d, int B, std::vector<double>& risk_rows);  // enqueues last_tighten and the round's risk rows
  void keep_tighten_risk(int B, const std::vector<double>& risk_rows);       // after the wait: their CR_STEP_RISK column
  void solve_tightened(const double x_0[4], Matrix& U, const double poly_coeffs[6], const double fl[2]);  // run_step's solve
  // map tightening (set_map_tightening): Sigma0, W and lamb are the tightening's above (the setters agree on them).  The map as it was
  // set, and, while the tightening is on, one device block of floats: the original layer, then a tightened layer per candidate
  bool map_tighten_ = false;
  int mt_rounds_ = 0;
  double mt_kappa_ = 0.0, mt_cap_ = 1.0;
  Uncertainty unc_;
  float* map_dev_ = nullptr;
  size_t map_dev_cap_ = 0;
  void apply_map(const Uncertainty& u);  // puts `u` on the handle: through map_dev_ while the map tightening is on
  cilqr_uncertainty_map device_map(bool tightened) const;  // the original in map_dev_, or the per-solve layers behind it
  double tightening_kappa(const char* setter, bool on, double eps, int rounds, double max_inflate) const;
  void check_tightening_agrees(bool other_on, int other_rounds, const double Sigma0[16], const double* W, double lamb, int rounds) const;
  // track map (set_track_map): its rounds run in tighten_rounds, its layers lie in map_dev_ behind the original
  int tm_rounds_ = 0, tm_window_ = 0;
  double tm_inflate_ = 0.0, tm_z_max_ = 0.0;
  bool tm_ellipses_ = true;
  int solve_obstacles() const;  // the M the SOLVES read: 0 under the track map with ellipses off
  void check_track_map_conflicts() const;  // throws std::logic_error, before a run enqueues anything
  bool map_in_block() const { return map_tighten_ || tm_rounds_ > 0; }  // the map lives in map_dev_
  // map obstacles (set_map_obstacles): the last map_rows_ entries of obstacles_ are last_map_obstacles over map_rows_horizon_ steps
  bool mo_on_ = false;
  double mo_threshold_ = 0.0, mo_gap_ = 0.0, mo_max_size_ = 0.0, mo_pad_ = 0.0;
  int mo_min_cells_ = 1, mo_K_ = 1, map_rows_ = 0, map_rows_horizon_ = -1;
  void* mo_dev_ = nullptr;
  size_t mo_dev_cap_ = 0;
  void extract_map_obstacles();                // unc_ -> last_map_obstacles, last_map_obstacle_counts
  void append_map_rows();                      // replaces the map's entries of obstacles_ by last_map_obstacles, packs
  void refresh_map_rows() { if (map_rows_ && map_rows_horizon_ != params.horizon) append_map_rows(); }  // (the horizon changed)
  void check_map_obstacle_conflicts() const;   // throws std::logic_error, before a run enqueues anything
  // map tracker (set_map_tracker): the table, the world record and the output rows live in trk_dev_; the detections are the boxes
  // extract_map_obstacles left in mo_dev_ (mo_boxes_dev_, mo_n_out_dev_)
  bool trk_on_ = false, trk_reset_ = true, trk_owns_tracks_ = false;
  cilqr_track_filter trk_f_{};
  int trk_slots_ = 0;
  void* trk_dev_ = nullptr;
  double* mo_boxes_dev_ = nullptr;
  int32_t* mo_n_out_dev_ = nullptr;
  void track_map_obstacles();  // one tick on the boxes in mo_dev_, then the confirmed rows installed as tracks
  void drop_tracker_tracks();  // removes what track_map_obstacles installed
  // mover clearing (set_mover_clearing): the layer as it was given is kept beside unc_, whose layer is then the cleared one; the call
  // reads the layer, the labels and comp in mo_dev_ and assign and the table in trk_dev_, and leaves its fields behind the pose in mo_dev_
  bool mv_on_ = false;
  double mv_v_clear_ = 0.0, mv_halo_ = 0.0;
  float mv_fill_ = 0.0f;
  std::vector<float> given_layer_;
  int mover_halo2(double res) const;  // throws std::runtime_error beyond CILQR_CLEAR_MOVERS_MAX_HALO2
  void clear_tracked_movers();        // mo_dev_, trk_dev_ -> unc_.layer, last_mover_clearing, the handle's map
};

}  // namespace cilqr_host
