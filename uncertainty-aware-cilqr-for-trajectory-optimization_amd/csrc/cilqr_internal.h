// cilqr_internal.h — shared between the C-ABI translation unit and the HIP kernels (not installed).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cilqr.h"
#include "cilqr_wave_plan.h"

namespace cilqr {

// Scalars the kernels need, derived once per handle from cilqr_params on the host (so that the libm calls
// tan(steer_angle_*) are the host's, exactly as in the reference, I/Model.cpp:20 / I/Constraints.cpp:119-121).
struct KParams {
  double dt;             // timestep
  double desired_speed;
  double tolerance;
  double w_acc, w_yawrate, w_pos, w_vel, w_obstacle;
  double q1_acc, q2_acc, q1_yawrate, q2_yawrate;
  double q1_front, q2_front, q1_rear, q2_rear;
  double acc_max, acc_min;
  double yaw_hi, yaw_lo;  // tan(steer_angle_max)/wheelbase, tan(steer_angle_min)/wheelbase: yaw-rate bound per unit speed
  double half_dt2;        // timestep²/2
  double wheelbase, speed_max;
  double t_safe, s_safe_a, s_safe_b, ego_rad, ego_front, ego_rear;
  double lamb_factor, lamb_max;
  int32_t max_iterations;
  int32_t n_samples;  // num_of_local_wpts * 10 (I/Constraints.cpp:28)
};

// The uncertainty map as the kernels read it (cilqr_set_uncertainty_map*, include/cilqr.h); layer == nullptr: no map set.
struct UncArgs {
  const float* layer;     // rows*cols float32 column-major per solve (stride floats apart; 0: shared)
  const double* poses;    // null, or [B][3] per-solve (x, y, theta) of the vehicle frame in the planning frame
  long long stride;
  int32_t rows, cols, nl, nw;
  double x_first, y_first, inv_res;  // centre of cell (0, 0) and 1/resolution (G/grid_map_core/src/GridMapMath.cpp:114-127)
  double px, py, cp, sp;             // shared pose: position, cos and sin of its heading (host libm)
  double la0, la_step, wb0, wb_step; // footprint probe offsets along / across the heading: la0 + k*la_step, wb0 + l*wb_step
  double q1, q2, scale;              // barrier constants; scale = w_uncertainty / (nl*nw)
};

constexpr int DIAG_SLOTS = 16;  // uint64 per solve in the diagnostic buffer (include/cilqr.h, cilqr_set_diag_buffer)

struct SolveArgs {
  const double* x0;
  double* U;
  const double* poly;
  const double* xplan_fl;
  const double* obs_pose;
  const double* obs_dim;
  const double* obs_weight;  // may be null
  // obstacle m of solve b at step t: pose + 4e, dim + 2e with e = b*obs_bs + m*obs_ms + t*obs_ts (entries; dense: M*N, N, 1);
  // weight of obstacle m of solve b: obs_weight[b*obs_wbs + m].  The sampled form keeps its dense nominal layout.
  long long obs_bs, obs_ms, obs_ts, obs_wbs;
  // 1: one scene for the batch, and obs_tab starts with ONE [M][N][6] table built in front of the solve kernels
  // (launch_obstacle_table) that every solve of the kernels keeping their table in the workspace reads and none writes
  int32_t obs_shared;
  double* X_out;
  double* J_out;        // may be null
  int32_t* iters_out;   // may be null
  int32_t* status_out;  // may be null
  const double* samp_off;  // sampled obstacles only: [B][M][n_samples][3] = (dx, dy, dtheta); then obs_pose/obs_dim are the
  int32_t n_samples;       // nominal trajectories of the M obstacles, every sample weighs samp_w, and the wavefront family runs.
  double samp_w;           // n_samples == 0: ordinary obstacles
  double* obs_tab;      // workspace: [B][M][N][6] (sampled: [B][M][N][8])
  double* fwd;          // workspace of the one-wavefront-per-solve family: [B][N + 1][16] forward-pass records (cilqr_solve.hip)
  int32_t* redo;        // workspace: [B] hand-over flags from the fast kernel to the general kernel
  unsigned long long* diag;  // null, or [B][DIAG_SLOTS] phase cycle totals (diagnostic instantiation)
  int32_t* passes;      // null, or [B]: backward+forward passes each solve actually executed (cilqr_set_pass_count_buffer)
  // Dispatch order of the one-wavefront-per-solve family for batches beyond one solve per SIMD (cilqr_api.cpp, schedule hint):
  const int32_t* order;  // null, or [B]: workgroup i runs solve order[i] (a permutation: longest solves of the previous call first)
  int32_t* hint_passes;  // null, or [B]: passes of each solve of THIS call, from which the next call's order is built
  int32_t B, N, M;
  uint32_t flags;
  // grouped family: 1 = in phase L the lanes of a wavefront's finished solves take steps of the unfinished ones (cilqr_solve_groups.hip)
  int32_t steal;
  KParams kp;
  UncArgs unc;
};

// Launchers (defined in the .hip files). All are asynchronous on `stream`.
// One wavefront per solve, LDS-resident (cilqr_solve.hip).
hipError_t launch_solve_wave(const SolveArgs& a, const WavePlan& plan, hipStream_t stream);  // carries out plan_wave's plan (cilqr_wave_plan.h)
hipError_t launch_schedule_order(const int32_t* passes, int B, int32_t* order, hipStream_t stream);  // passes descending
// G lanes per solve (G in {1,2,4,8,16,32}), workspace `ws` of solve_groups_ws_doubles(B, N) doubles (cilqr_solve_groups.hip).
hipError_t launch_solve_groups(const SolveArgs& a, int G, double* ws, hipStream_t stream);
size_t solve_groups_ws_doubles(int B, int N);
// One scene for the batch (a.obs_shared): the M·N entries of solve 0's obstacle table → a.obs_tab[(m*N + t)*6 ...] (obstacle_table.hip)
hipError_t launch_obstacle_table(const SolveArgs& a, hipStream_t stream);
// Test hook: the map cost alone at n states [n][4] → cost[n], vx[n][2], mx[n][3] (solve 0's layer and pose).
hipError_t launch_unc_cost(const UncArgs& u, int n, const double* states, double* cost, double* vx, double* mx, hipStream_t stream);
hipError_t launch_quu_inverse(int n, const double* q, const double* lamb, double* out, int general, hipStream_t stream);
hipError_t launch_closest_sample(int n, int S, const double* in, int32_t* out, hipStream_t stream);  // test hook (cilqr_debug_closest_sample)
// Test hook (cilqr_debug_math): exp_fast, sincos_fast, sincos_loop or a rotate_heading chain of T steps on n rows, one lane per row.
hipError_t launch_debug_math(const KParams& kp, int op, int n, int T, const double* in, double* out, hipStream_t stream);

// Scoring of solved trajectories (cilqr_score.hip; cilqr_score_batch*, include/cilqr.h): one workgroup of SCORE_THREADS lanes per
// solve.  `s` carries what the launch shares with a solve — U, poly, xplan_fl, the obstacle fields (strided, or the compact sampled
// form with M = nominal obstacles and n_samples > 0), B, N, M, kp, unc — and the trajectories to score in X_out (read only).
constexpr int SCORE_THREADS = 256;
constexpr size_t SCORE_LDS_MAX = 64 * 1024;  // dynamic LDS a launch gets without opting in to more
struct ScoreArgs {
  SolveArgs s;
  double* score;         // [B][CILQR_SCORE_FIELDS]
  double* total;         // [B] or null
  double max_collision;
  double w_uncertainty;  // Parameters::w_uncertainty (UncArgs::scale holds it divided by the probe count only)
  // rows per solve (cilqr_score_rollouts: s.B counts ROWS, row r reads X_out / U at r and everything else of solve r / rows); the
  // score calls pass 1
  int32_t rows;
};
hipError_t launch_score(const ScoreArgs& a, hipStream_t stream);
size_t score_lds_bytes(int N, int S, int n_counters);  // n_counters: n_obs·N per-(t, o) sample counters of the sampled form, else 0
// Each solve's S score rows → risk [B][CILQR_RISK_FIELDS], total [B] or null (cilqr_score.hip): one wavefront per solve.
struct RiskArgs {
  const double* row_score;  // [B·S][CILQR_SCORE_FIELDS]
  double* risk;
  double* total;
  double max_risk;
  int32_t B, S;
};
hipError_t launch_risk(const RiskArgs& a, hipStream_t stream);

// One backward pass at a given trajectory (cilqr_gains.hip; cilqr_gains_batch*): one wavefront per solve.  `s` carries what the
// launch shares with a solve — X_out = the trajectory (read only), U, poly, xplan_fl, the strided obstacle fields (or the compact
// sampled form with M = nominal obstacles and n_samples > 0), B, N, M, kp, unc.
struct GainsArgs {
  SolveArgs s;
  double* k_out;    // [B][2N]
  double* K_out;    // [B][8N], K[8t + r + 2c]
  int32_t* ok_out;  // [B] or null
  double lamb;
};
hipError_t launch_gains(const GainsArgs& a, hipStream_t stream);
size_t gains_lds_bytes(int N, int n_path_samples);
constexpr size_t GAINS_LDS_MAX = 64 * 1024;

// S closed-loop rollouts per solve (cilqr_rollout.hip; cilqr_rollout_batch*): lane = sample, a wavefront holds up to 64 samples of
// one solve.
struct RolloutArgs {
  const double *X, *U, *k, *K;  // nominal trajectory and gains, [B][…]
  const double* delta;          // [B or 1][S][4]
  long long delta_bs;           // doubles between two solves' offset sets (0: shared)
  double* X_roll;               // [B·S][4(N+1)]
  double* U_roll;               // [B·S][2N]
  double k_scale;
  int32_t B, N, S;
  KParams kp;
};
hipError_t launch_rollout(const RolloutArgs& a, hipStream_t stream);
size_t rollout_lds_bytes(int N);

// Collision risk of S closed-loop rollouts per solve with no rollout stored (cilqr_risk.hip; cilqr_rollout_risk*): lane = rollout
// row, a workgroup holds up to RISK_THREADS rows of one solve, solve b has G = ceil(S / RISK_THREADS) workgroups.  `s` carries what
// the launch shares with a solve — the strided obstacle fields, B, N, M, kp — and comes first, so that phase_args / phase_params
// of cilqr_device.hpp read it.
constexpr int RISK_THREADS = 256;
constexpr int RISK_WAVES = RISK_THREADS / 64;
constexpr int RISK_PART_DOUBLES = 8;  // doubles at the head of a partial record; N int32 step counts follow
constexpr size_t RISK_LDS_MAX = 64 * 1024;
struct RolloutRiskArgs {
  SolveArgs s;
  const double *X, *U, *k, *K;  // nominal trajectory and gains, [B][…]
  const double* delta;          // [B or 1][S][4]
  long long delta_bs;           // doubles between two solves' offset sets (0: shared)
  double k_scale, max_risk;
  const double* base;           // [B] or null (then total is null)
  double* risk;                 // [B][CILQR_ROLLOUT_RISK_FIELDS]
  int32_t* step_hits;           // [B][N] or null
  double* total;                // [B] or null
  double* partials;             // the handle's: B·G records, part_stride doubles apart (read and written for G > 1 only)
  long long part_stride;
  int32_t S, G;
};
hipError_t launch_rollout_risk(const RolloutRiskArgs& a, hipStream_t stream);
size_t rollout_risk_lds_bytes(int N, int M);
// The same against sampled obstacles in compact form (cilqr_risk_sampled.hip; cilqr_rollout_risk_sampled*): `s` carries the dense
// nominal tables, M = n_obs, samp_off and n_samples > 0; risk has CILQR_RRS_FIELDS per solve.  For G > 1 `partials` holds B·G
// records, part_stride = rollout_risk_sampled_part_doubles(N, n_obs) doubles apart: 8 doubles, then N + N·n_obs int32 counters.
hipError_t launch_rollout_risk_sampled(const RolloutRiskArgs& a, hipStream_t stream);
size_t rollout_risk_sampled_lds_bytes(int N, int n_obs, int n_samples);
size_t rollout_risk_sampled_part_doubles(int N, int n_obs);
// The same against the uncertainty map set on the handle (cilqr_risk_map.hip; cilqr_rollout_risk_map*): `r.s` carries B, N, kp and
// unc (no obstacle field is read); risk has CILQR_MAP_RISK_FIELDS per solve.  For G > 1 `r.partials` holds B·G records of the
// cilqr_rollout_risk shape — 8 doubles, then N int32 — whose counters pack the unknown rows above the hit rows (16 bits each).
struct MapRiskArgs {
  RolloutRiskArgs r;
  double occ_threshold;
  int32_t* unknown_hits;  // [B][N] or null
  uint32_t flags;         // CILQR_MAP_RISK_*
};
hipError_t launch_rollout_risk_map(const MapRiskArgs& a, hipStream_t stream);
size_t rollout_risk_map_lds_bytes(int N);

// Analytic map risk (cilqr_chance_map.hip; cilqr_chance_risk_map*): quadrature nodes placed through the factor of Sigma_t's pose
// marginal, looked up in the uncertainty map set on the handle.  lane = node, wavefront = step, a workgroup takes
// CHANCE_MAP_WAVES consecutive steps of one solve, solve b has G = ceil(N / CHANCE_MAP_WAVES) workgroups; a finish kernel, one
// wavefront per solve, reduces over the steps.  `s` carries B, N and unc.  The three per-step pointers are never null: the
// caller's arrays, or the handle's.  `partials`: the handle's, one record of part_stride doubles per solve whose first G hold the
// workgroups' largest occupancies.
constexpr int CHANCE_MAP_WAVES = 4;
constexpr int CHANCE_MAP_THREADS = 64 * CHANCE_MAP_WAVES;
struct ChanceMapArgs {
  SolveArgs s;
  const double *X, *sigma;        // [B][4(N + 1)], [B][N + 1][16]
  const double *nodes, *weights;  // [Q][3], [Q]
  double occ_threshold, max_risk;
  const double* base;             // [B] or null (then total is null)
  double* risk;                   // [B][CILQR_CHANCE_MAP_FIELDS]
  double *step_risk, *step_occ, *step_unknown;  // [B][N] each
  double* total;                  // [B] or null
  double* partials;
  long long part_stride;
  int32_t Q, G;
  uint32_t flags;                 // CILQR_CHANCE_MAP_*
};
hipError_t launch_chance_risk_map(const ChanceMapArgs& a, hipStream_t stream);
size_t chance_risk_map_lds_bytes(int Q);

// Analytic chance risk against sampled obstacles in compact form (cilqr_chance_sampled.hip; cilqr_chance_risk_sampled*): the
// mapping of the map kernel above — wavefront = step, a workgroup takes CHANCE_SAMPLED_WAVES consecutive steps of one solve, solve b
// has G = ceil(N / CHANCE_SAMPLED_WAVES) workgroups, lanes take the step's n_obs·n_samples entries; a finish kernel, one wavefront
// per solve, reduces over the steps.  `s` carries the dense nominal tables, M = n_obs, samp_off, n_samples > 0, B, N and kp.
// `steps`: the handle's, one record of CHANCE_SAMPLED_REC doubles per (solve, step).
constexpr int CHANCE_SAMPLED_WAVES = 4;
constexpr int CHANCE_SAMPLED_THREADS = 64 * CHANCE_SAMPLED_WAVES;
constexpr int CHANCE_SAMPLED_REC = 5;
struct ChanceSampledArgs {
  SolveArgs s;
  const double *X, *sigma;               // [B][4(N + 1)], [B][N + 1][16]
  double max_risk;
  const double* base;                    // [B] or null (then total is null)
  double* risk;                          // [B][CILQR_CRS_FIELDS]
  double *step_risk, *pair_p, *entry_p;  // [B][N], [B][n_obs][N], [B][n_obs·n_samples][N]; each may be null
  double* total;                         // [B] or null
  double* steps;
  int32_t G;
  uint32_t flags;                        // CILQR_CHANCE_SAMPLED_*
};
hipError_t launch_chance_risk_sampled(const ChanceSampledArgs& a, hipStream_t stream);
size_t chance_risk_sampled_lds_bytes(int n_obs, int n_samples);  // 8 bytes per entry of a step and wavefront, whatever N is
constexpr size_t CHANCE_SAMPLED_LDS_MAX = 64 * 1024;

// Closed-loop covariance chain and Gaussian chance values per solve (cilqr_chance.hip; cilqr_chance_risk*): one workgroup per
// solve.  `s` carries what the launch shares with a solve — the strided obstacle fields, B, N, M, kp — and comes first, so that
// phase_args / phase_params of cilqr_device.hpp read it.
constexpr int CHANCE_THREADS = 256;
constexpr size_t CHANCE_LDS_MAX = 64 * 1024;
struct ChanceArgs {
  SolveArgs s;
  const double *X, *U, *K;   // the plan and its gains, [B][…]
  const double* sigma0;      // [B or 1][16]
  long long sigma0_bs;       // doubles between two solves' Σ0 (0: shared)
  const double* W;           // [16] or null (zero)
  double max_risk;
  const double* base;        // [B] or null (then total is null)
  double* risk;              // [B][CILQR_CHANCE_FIELDS]
  double* step_risk;         // [B][N] or null
  double* entry_p;           // [B][M·N] or null
  double* sigma_out;         // [B][N + 1][16] or null
  double* total;             // [B] or null
  uint32_t flags;            // CILQR_CHANCE_*
};
hipError_t launch_chance_risk(const ChanceArgs& a, hipStream_t stream);
// cilqr_chance_risk_cov: the same with the obstacles' own covariance, (xx, xy, yy) at obs_cov + 3e for the obstacle entry index e,
// for the kernel's second instantiation (ChanceArgs stays as it is: so does the argument segment of the first)
struct ChanceCovArgs : ChanceArgs {
  const double* obs_cov;     // never null
};
template <bool COV> struct ChanceKernelArgs { typedef ChanceArgs type; };
template <> struct ChanceKernelArgs<true> { typedef ChanceCovArgs type; };
hipError_t launch_chance_risk_cov(const ChanceCovArgs& a, hipStream_t stream);
size_t chance_risk_lds_bytes(int N, int M);

// Constant-acceleration, constant-yaw-rate prediction of tracked obstacles with their covariance (cilqr_predict.hip;
// cilqr_predict_obstacles*): one wavefront per track, `tracks` = T·M workgroups.
constexpr int PREDICT_THREADS = 64;
constexpr size_t PREDICT_LDS_MAX = 64 * 1024;
struct PredictArgs {
  const double* track;      // [tracks][6]
  const double* track_dim;  // [tracks][2]
  const double* track_cov;  // [tracks][16] or null (zero)
  const double* noise;      // [16] or null (zero)
  double* pose_out;         // [tracks][4N]
  double* dim_out;          // [tracks][2N]
  double* cov_out;          // [tracks][N][3] or null
  double* sigma_out;        // [tracks][N][16] or null
  double dt, half_dt2;
  int32_t N;
  long long tracks;
};
hipError_t launch_predict_obstacles(const PredictArgs& a, hipStream_t stream);
size_t predict_lds_bytes(int N);

// One tick of the obstacle tracker (cilqr_track.hip; cilqr_track_update*): one wavefront per world, W workgroups.  The filter
// travels by value in the kernel arguments.
constexpr int TRACK_THREADS = 64;
struct TrackArgs {
  const double* det;        // [W][D][5] or null (D = 0)
  const int32_t* n_det;     // count of world w at [w·n_det_stride], or null (D)
  const double* state_in;   // [W][M][CILQR_TRACK_STATE]; not read under CILQR_TRACK_RESET
  double* state_out;        // [W][M][CILQR_TRACK_STATE]; may equal state_in
  double* world;            // [W][CILQR_TRACK_WORLD_FIELDS]
  int32_t* assign;          // [W][D] or null
  double* track_out;        // [W][M][6]
  double* dim_out;          // [W][M][2]
  double* cov_out;          // [W][M][16]
  long long n_det_stride;
  cilqr_track_filter f;
  int32_t W, M, D;
  uint32_t flags;           // CILQR_TRACK_*
};
hipError_t launch_track_update(const TrackArgs& a, hipStream_t stream);

// Chance-constraint tightening (cilqr_tighten.hip; cilqr_tighten_obstacles*): every obstacle entry's dimensions grown by kappa
// standard deviations of the relative position along the ellipse's axes.  One workgroup per solve; `s` first, as in ChanceArgs.
constexpr int TIGHTEN_THREADS = 256;
constexpr size_t TIGHTEN_LDS_MAX = 64 * 1024;
struct TightenArgs {
  SolveArgs s;
  const double* X;        // [B][4(N + 1)]
  const double* sigma;    // [B][N + 1][16], sigma_out of the chance risk
  const double* obs_cov;  // null (zero), or (xx, xy, yy) at obs_cov + 3e for the obstacle entry index e
  double kappa, max_inflate;
  double* pose_out;       // [B][M][4N] or null
  double* dim_out;        // [B][M][2N]
  double* tighten;        // [B][CILQR_TIGHTEN_FIELDS]
};
hipError_t launch_tighten_obstacles(const TightenArgs& a, hipStream_t stream);
size_t tighten_lds_bytes(int N);

// Map tightening (cilqr_tighten_map.hip; cilqr_tighten_map*): the layer set on the handle dilated, per cell, by kappa standard
// deviations of the footprint point over that cell, taken from the Sigma_t of the plan's nearest step.  lane = cell; solve b has G
// workgroups of TIGHTEN_MAP_THREADS lanes that stride over its cells; a finish kernel, one wavefront per solve, merges the G
// records of TIGHTEN_MAP_REC doubles each workgroup leaves in `partials`.  `s` carries B, N and unc.
constexpr int TIGHTEN_MAP_THREADS = 256;
constexpr int TIGHTEN_MAP_REC = 5;   // raised count, largest raise, its cell, largest reach, capped count
constexpr int TIGHTEN_MAP_MAX_G = 64;  // workgroups per solve at most: the node's 150 x 100 map is 59 tiles of 256 cells
constexpr int TIGHTEN_MAP_STEP = 8;  // doubles per step in LDS: p_t and six map-frame covariance entries
struct TightenMapArgs {
  SolveArgs s;
  const double *X, *sigma;  // [B][4(N + 1)], [B][N + 1][16]
  double kappa, max_inflate;
  double res, r_fp;         // the map's resolution as it was set; half the footprint's diagonal
  float* layer_out;         // [B][rows·cols]
  double* tighten;          // [B][CILQR_TIGHTEN_MAP_FIELDS]
  double* partials;         // the handle's: B·G records of TIGHTEN_MAP_REC doubles
  int32_t G;
};
hipError_t launch_tighten_map(const TightenMapArgs& a, hipStream_t stream);
size_t tighten_map_lds_bytes(int N);

// Predicted tracks rasterised into the map along each plan (cilqr_track_map.hip; cilqr_rasterize_tracks*): per solve a copy of the
// layer set on the handle, every cell raised to 100 x the probability that a predicted vehicle covers it.  Three launches:
//   records  one lane per entry e = m·N + t: the entry's record of TRACK_MAP_ENTRY doubles in the planning frame, into `records`;
//            `sets` = 1 record set when the obstacles' batch stride is 0, else one per solve
//   cells    lane = cell; solve b has G workgroups of TRACK_MAP_THREADS lanes that stride over its cells (the G of the map
//            tightening: a function of the map alone) and leave one record of TRACK_MAP_REC doubles each in `partials`
//   finish   one wavefront per solve merges the G records and counts the lost entries
// `s` carries B, N, M, the strided obstacle fields and unc.
constexpr int TRACK_MAP_THREADS = 256;
constexpr int TRACK_MAP_ENTRY = 10;  // o.x, o.y, cos, sin, hl, hw, 1/(su·sqrt 2), 1/(sw·sqrt 2), reach along, reach across (-1: lost)
constexpr int TRACK_MAP_REC = 4;     // raised count, largest v, its cell, the entry that gave it
constexpr int TRACK_MAP_MAX_G = 64;
constexpr int TRACK_MAP_STEP = 2;    // doubles per plan step in LDS: p_t in the map frame
constexpr int TRACK_MAP_POSE = 4;    // doubles of the solve's map pose in LDS: position, cos and sin of its heading
constexpr size_t TRACK_MAP_LDS_MAX = 64 * 1024;
struct TrackMapArgs {
  SolveArgs s;
  const double* X;         // [B][4(N + 1)], or null: swept mode
  const double* obs_cov;   // null (zero), or (xx, xy, yy) at obs_cov + 3e for the obstacle entry index e
  double inflate, z_max;
  double res;              // the map's resolution as it was set
  float* layer_out;        // [B][rows·cols]
  double* fields;          // [B][CILQR_TRACK_MAP_FIELDS]
  double* records;         // the handle's: sets·M·N records of TRACK_MAP_ENTRY doubles
  double* partials;        // the handle's: B·G records of TRACK_MAP_REC doubles
  int32_t G, window, sets; // window already clamped to N
  uint32_t flags;          // CILQR_TRACK_MAP_*
};
hipError_t launch_rasterize_tracks(const TrackMapArgs& a, hipStream_t stream);
size_t track_map_lds_bytes(int N);

// Exact footprint check (cilqr_footprint.hip; cilqr_footprint_check*): the vehicle's rectangle against the obstacle rectangles and
// against the cells of the map set on the handle.  Three launches:
//   boxes  one workgroup of FOOTPRINT_THREADS lanes per row; lanes stride over the entries e = m·N + t
//   map    wavefront = (row, step), FOOTPRINT_WAVES steps per workgroup, rows·ceil(N / FOOTPRINT_WAVES) workgroups; lanes stride
//          over the virtual cells of the footprint's bounding box, i fastest (only when a map is set and not skipped)
//   merge  one wavefront per row folds the N step records and the boxes' record into fp and total
// `s` carries B (SOLVES), N, M, the strided obstacle fields and unc; row r = b·S + s reads X at r and everything else of solve b.
// `steps`: the handle's, one record of FOOTPRINT_STEP_REC doubles per (row, step) — boxes writes field 0, map fields 1..5 — then,
// behind rows·N records, FOOTPRINT_ROW_REC doubles per row (the boxes' smallest clearance and its entry) and, behind those, rows·N
// doubles that stand in for a step_clearance the caller did not ask for.
constexpr int FOOTPRINT_THREADS = 256;
constexpr int FOOTPRINT_WAVES = 4;
constexpr int FOOTPRINT_STEP_REC = 6;  // box hit, largest occupancy (-inf: none), its cell, cells above the threshold, hit | unknown << 1, covered cells
constexpr int FOOTPRINT_ROW_REC = 2;
constexpr size_t FOOTPRINT_LDS_MAX = 64 * 1024;
struct FootprintArgs {
  SolveArgs s;
  const double* X;         // [rows][4(N + 1)]
  double hl, hw;           // half-extents of the ego rectangle, the margin included
  double min_clearance, occ_threshold;
  double res;              // the map's resolution as it was set
  const double* base;      // [rows] or null (then total is null)
  double* fp;              // [rows][CILQR_FOOTPRINT_FIELDS]
  double* step_clearance;  // [rows][N]: the caller's, or the handle's
  float* step_occ;         // [rows][N] or null
  double* total;           // [rows] or null
  double *steps, *row_rec;
  int32_t rows, S, map_on;
  uint32_t flags;          // CILQR_FOOTPRINT_*
};
hipError_t launch_footprint_check(const FootprintArgs& a, hipStream_t stream);
size_t footprint_lds_bytes(int N);
inline size_t footprint_scratch_doubles(size_t max_batch, size_t max_horizon) {
  return max_batch * max_horizon * (FOOTPRINT_STEP_REC + 1) + max_batch * FOOTPRINT_ROW_REC;
}

// Distance to the occupied cells of a layer (costmap_distance.hip; cilqr_map_distance*, cilqr_inflate_map*).  Two launches for the
// field — lane = row, walking the columns; then one workgroup per (layer, column) with the column in LDS — and one, lane = cell,
// for the inflated layer.  Layers are `layer_stride` floats apart (0: one shared layer); outputs are dense, rows·cols apart.
constexpr int MAP_DISTANCE_THREADS = 256;
constexpr int MAP_DISTANCE_MAX_SIDE = 8192;  // rows, cols at most: d2 <= 2·8192² < 2^31, and a column of int32 is 32 KiB of LDS
struct MapDistanceArgs {
  const float* layer;
  long long layer_stride;
  int32_t* d2_out;   // [L][rows·cols]
  float* dist_out;   // [L][rows·cols] or null
  double occ_threshold, res;
  int32_t L, rows, cols;
  uint32_t flags;    // CILQR_MAP_DISTANCE_*
};
hipError_t launch_map_distance(const MapDistanceArgs& a, hipStream_t stream);
struct InflateMapArgs {
  const float* layer;
  long long layer_stride;
  const int32_t* d2;  // [L][rows·cols]
  float* layer_out;   // [L][rows·cols]
  double res, inscribed, radius, peak;
  int32_t L, rows, cols;
};
hipError_t launch_inflate_map(const InflateMapArgs& a, hipStream_t stream);

// Connected components of the linked cells of L distance fields, and their boxes (costmap_components.hip; cilqr_map_obstacles*).
// Seven launches behind one 16·L-byte clear of n_out: tiles (union-find in LDS), seams (global atomic minima), flatten + count,
// rank (one workgroup per layer), moments (lane = linked cell, integer atomics into the slot's row of comp), extents (one workgroup
// per slot), finish (one workgroup per layer: filter, compact, filler rows).  Everything is dense, rows·cols or K rows apart.
constexpr int MAP_OBSTACLES_THREADS = 256;
constexpr int MAP_OBSTACLES_RANK_THREADS = 1024;
constexpr int MAP_OBSTACLES_MAX_SIDE = 1024;  // rows, cols at most: every term of c·Sii - Si² stays within 2^60
struct MapObstaclesArgs {
  const int32_t* d2;   // [L][rows·cols]
  const double* pose;  // [L or 1][3] or null
  int32_t* work;       // [L][rows·cols]
  int32_t* label_out;  // [L][rows·cols]
  int32_t* n_out;      // [L][4]
  double* comp;        // [L][K][CILQR_MAP_OBSTACLE_FIELDS]
  double* boxes;       // [L][K][5] or null
  double* pose_out;    // [L][K][4] or null
  double* dim_out;     // [L][K][2] or null
  double res, x_first, y_first, max_size, pad;
  int32_t L, rows, cols, gap2, K, min_cells, pose_stride;
  uint32_t flags;      // CILQR_MAP_OBSTACLES_*
};
hipError_t launch_map_obstacles(const MapObstaclesArgs& a, hipStream_t stream);

// Static layer: the cells of the components that moving tracks own, taken out of L layers (costmap_movers.hip; cilqr_clear_movers*).
// One 64·L-byte clear of `fields`, one launch with a workgroup per 64 x 16 tile (layer slowest) that adds its counts into `fields`
// as raw 64-bit integers, and one launch, lane = layer, that turns them into doubles.  Outputs are dense, rows·cols apart.
constexpr int CLEAR_MOVERS_THREADS = 256;
struct ClearMoversArgs {
  const float* layer;
  long long layer_stride;
  const int32_t* label;   // [L][rows·cols]
  const double* comp;     // [L][K][CILQR_MAP_OBSTACLE_FIELDS]
  const int32_t* assign;  // [L][K], tracker form; null in the mask form
  const double* state;    // [L][M][CILQR_TRACK_STATE], tracker form
  const int32_t* mask;    // [L][K], mask form; null in the tracker form
  float* layer_out;       // [L][rows·cols]
  int32_t* owner_out;     // [L][rows·cols] or null
  double* fields;         // [L][CILQR_CLEAR_MOVERS_FIELDS]
  double v_clear;
  float fill;
  int32_t L, rows, cols, K, M, min_hits, halo2, r;
};
hipError_t launch_clear_movers(const ClearMoversArgs& a, hipStream_t stream);
size_t clear_movers_lds_bytes(int K, int r);

// Exact clearance of the ego rectangle to the occupied cells of the map set on the handle (cilqr_map_clearance.hip;
// cilqr_map_clearance*).  Two launches: wavefront = (row, step), FOOTPRINT_WAVES steps per workgroup, lanes over the cells of the
// window; then one wavefront per row for the fold.  `s` carries B (SOLVES), N and unc; row r = b·S + s reads X at r and the layer and
// pose of solve b.  `steps`: the handle's footprint region (footprint_scratch_doubles), here one record of MAP_CLEARANCE_STEP_REC
// doubles per (row, step) and, behind max_batch·max_horizon of them, rows·N doubles that stand in for a step_clearance the caller
// did not ask for.
constexpr int MAP_CLEARANCE_STEP_REC = 2;  // the step's nearest cell (-1: none), window leaves the map | lost << 1
struct MapClearanceArgs {
  SolveArgs s;
  const double* X;         // [rows][4(N + 1)]
  double hl, hw;           // half-extents of the ego rectangle, the margin included
  double reach, min_clearance, occ_threshold;
  double res;              // the map's resolution as it was set
  const double* base;      // [rows] or null (then total is null)
  double* mc;              // [rows][CILQR_MAP_CLEARANCE_FIELDS]
  double* step_clearance;  // [rows][N]: the caller's, or the handle's
  double* total;           // [rows] or null
  double* steps;
  int32_t rows, S;
  uint32_t flags;          // CILQR_MAP_CLEARANCE_*
};
hipError_t launch_map_clearance(const MapClearanceArgs& a, hipStream_t stream);

// Stop plans (cilqr_stop.hip; cilqr_stop_plans*): row r = b·D + l is plan b braked at level l.  One launch of STOP_THREADS lanes per
// workgroup; a workgroup holds `plans` plans (stop_plans_per_group) and the rows of up to 64 levels of each.
constexpr int STOP_THREADS = 256;
constexpr int STOP_WAVES = 4;
constexpr size_t STOP_LDS_MAX = 64 * 1024;
struct StopArgs {
  const double* X;          // [B][4(N + 1)]
  const double* U;          // [B][2N]
  const double* decel;      // [D]
  const double* plan_cost;  // [B] or null
  double* X_stop;           // [B·D][4(N + 1)]
  double* U_stop;           // [B·D][2N]
  double* sp;               // [B·D][CILQR_STOP_FIELDS]
  double* cost;             // [B·D] or null
  double max_deviation, decel_weight;
  int32_t B, N, D, hold;
  int32_t plans;            // plans per workgroup
  uint32_t flags;           // CILQR_STOP_*
  double dt, half_dt2, acc_max, acc_min, yaw_hi, yaw_lo, speed_max;  // the model's constants (KParams)
};
int stop_plans_per_group(int N, int D);  // at least 1 for every N <= CILQR_MAX_HORIZON
hipError_t launch_stop_plans(const StopArgs& a, hipStream_t stream);

// Batched LocalPlanner (local_plan.hip): one lane per candidate.
struct LocalPlanArgs {
  const double* path;      // 2×P column-major; candidate b reads path + b*path_stride (0: one shared path)
  long long path_stride;   // in doubles
  const double* ego;       // [B][4]
  double* poly;            // [B][6]
  double* xplan_fl;        // [B][2]
  double* ref_traj;        // null or [B][2*n_wpts]
  int32_t* n_out;          // null or [B]
  int32_t B, P, n_wpts, cols;
};
hipError_t launch_local_plan(const LocalPlanArgs& a, hipStream_t stream);
size_t local_plan_lds_bytes(int n_wpts, int cols);

// The same pre-step in the path-aligned frame of each candidate (include/cilqr.h, "path-aligned planning frame"): the frame
// is chosen from the slice, the slice is taken into it and the fit runs on the framed abscissae.
struct LocalPlanFramesArgs {
  LocalPlanArgs p;      // ref_traj and xplan_fl receive frame coordinates
  double* frames;       // [B][CILQR_FRAME_DOUBLES]
  int32_t* info;        // [B] CILQR_FRAME_* bits
  double* ego_out;      // [B][4]
  int32_t* first_out;   // null or [B]
};
hipError_t launch_local_plan_frames(const LocalPlanFramesArgs& a, hipStream_t stream);

// Rigid transforms into and out of the frames (cilqr_frame.hip): one lane per entry, per (row, step), per pose.
struct FrameObstaclesArgs {
  const double* frames;   // solve b reads frames + b*frame_stride
  const double* pose;     // entries addressed by the strides below (cilqr_obstacles)
  const double* dim;
  const double* cov;      // null or 3 doubles per entry
  double* pose_out;       // [B][M][4N]
  double* dim_out;        // [B][M][2N]
  double* cov_out;        // null or [B][M][3N]
  long long bs, ms, ts;
  double two_t_safe;      // 2·t_safe
  int32_t B, N, M, frame_stride;
  uint32_t flags;
};
hipError_t launch_frame_obstacles(const FrameObstaclesArgs& a, hipStream_t stream);
struct FrameStatesArgs {
  const double* frames;
  const double* X_in;     // [B·S][4(N + 1)]
  double* X_out;          // may be X_in
  long long rows;         // B·S
  int32_t S, N, frame_stride, direction;
};
hipError_t launch_frame_states(const FrameStatesArgs& a, hipStream_t stream);
struct FramePosesArgs {
  const double* frames;
  const double* pose_in;  // solve b reads pose_in + b*pose_stride
  double* pose_out;       // [B][K][3]
  long long pose_stride;
  int32_t B, K, frame_stride;
};
hipError_t launch_frame_poses(const FramePosesArgs& a, hipStream_t stream);

// Min-cost selection (cilqr_select.hip).  out_pair {J_min, index} and/or out_triple {J_min, index, offset} (either may be null).
hipError_t launch_argmin(const double* J, int B, double* out_pair, double* out_triple, double offset, hipStream_t stream,
                         double pair_offset = 0.0);
hipError_t launch_select(const double* triples, int n_ranks, double* out_pair, hipStream_t stream);

struct WarpArgs {
  const float* src;
  float* dst;
  const float* bbox;  // may be null
  unsigned long long* n_oob;  // may be null
  cilqr_map_geom sg, dg;
  double vx, vy, sin_t, cos_t;
};
hipError_t launch_warp(const WarpArgs& a, hipStream_t stream);
// K frames per launch: poses [K][4] = (vx, vy, sin theta, cos theta) on the device, destination frames back to back, n_oob [K] or
// null.  Rows in fours take the 16-byte-store kernel, any other row count the cell-by-cell kernel with a frame dimension.
struct WarpBatchArgs {
  const float* src;
  float* dst;
  const float* bbox;          // may be null (one layer, shared by the frames)
  unsigned long long* n_oob;  // may be null
  const double* poses;        // null: ONE frame, its pose in pose0 (no table to upload)
  double pose0[4];
  cilqr_map_geom sg, dg;
};
hipError_t launch_warp_batch(const WarpBatchArgs& a, int K, hipStream_t stream);

// Obstacle polygons on the device (layout: costmap_polygons.hpp): n polygons of V vertices that can touch the map.
struct PolygonTable {
  const double* table;
  int32_t n, V;
};
constexpr size_t POLYGON_TABLE_DOUBLES = (size_t)CILQR_MAX_POLYGONS * (2 + 2 * CILQR_MAX_POLYGON_VERTICES);  // one full table
// Polygon::isInside of every cell centre (costmap_polygons.hip): value inside any polygon; elsewhere NaN (clear) or untouched.
hipError_t launch_rasterize_polygons(const PolygonTable& t, const cilqr_map_geom& g, float value, bool clear, float* layer, hipStream_t stream);
// launch_warp with the override decided by the polygons themselves (a.bbox is ignored): a covered cell takes 100, as if a.bbox
// were launch_rasterize_polygons(t, a.dg, 100, clear) — no such layer is written or read.
hipError_t launch_warp_polygons(const WarpArgs& a, const PolygonTable& t, hipStream_t stream);

struct BlurArgs {
  const float* src;
  float* out;
  int32_t* count_out;  // may be null
  int8_t* occ_out;     // may be null: the same cells as an OccupancyGrid (toOccupancyGrid of `out`, reversed order)
  float occ_min, occ_den;  // dataMin and dataMax - dataMin of that conversion
  cilqr_map_geom g;
  int32_t index;       // first linear cell index processed (cells before it are set NaN)
  double sin_t, cos_t, sigma_x, sigma_y, sigma_theta;
};
hipError_t launch_blur(const BlurArgs& a, hipStream_t stream);
// the argument block of a batched blur launch, and the kernel's argument type by instantiation (named at namespace scope so that
// the kernels' demangled names carry no nested parentheses: tools/compare_kernel_isa.py cuts them at the parameter list)
struct BlurBatchArgs {
  BlurArgs a;
  const double* poses;
  long src_stride;
};
template <bool FRAMES>
struct BlurKernelArgs { using type = BlurArgs; };
template <>
struct BlurKernelArgs<true> { using type = BlurBatchArgs; };
// K frames per launch: frame k reads a.src + k*src_stride (floats), takes (sin, cos) from poses[4k+2], poses[4k+3] (device table,
// the layout of WarpBatchArgs::poses; a.sin_t / a.cos_t are ignored) and writes a.out / a.occ_out / a.count_out + k*rows*cols.
hipError_t launch_blur_batch(const BlurArgs& a, int K, const double* poses, long src_stride, hipStream_t stream);
// OccupancyGrid <-> layer (costmap_occupancy.hip)
hipError_t launch_occ_to_layer(const int8_t* occ, float* layer, long n, hipStream_t stream);
// steps_ws: 102 floats of device workspace for the step table of large conversions (null: always the per-cell division)
hipError_t launch_layer_to_occ(const float* layer, int8_t* occ, long n, float data_min, float data_max, float* steps_ws,
                               hipStream_t stream);
hipError_t launch_blur_ellipse(int n, const double* abc, double* out, hipStream_t stream);

}  // namespace cilqr
