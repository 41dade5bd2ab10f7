// ilqr_adapter.cpp — see ilqr_adapter.h.  Host C++ over the C-ABI; the HIP runtime is used for one thing only: the device block
// and the stream of the pose-noise check (set_pose_noise_check), whose pipeline stays on the device between the C-ABI's _device calls.
#include "ilqr_adapter.h"

#include <hip/hip_runtime.h>

#include <string.h>

#include <stdexcept>
#include <string>

namespace cilqr_host {

namespace {
void check(int rc, const char* what) {
  if (rc != CILQR_OK) throw std::runtime_error(std::string(what) + ": " + cilqr_last_error());
}
}  // namespace

Parameters default_parameters() {
  Parameters p;
  cilqr_params_default(&p);
  return p;
}

iLQR::iLQR(const Parameters& params, int device, int max_obstacles, int max_candidates)
    : params(params), device_(device), max_obstacles_(max_obstacles), max_candidates_(max_candidates < 1 ? 1 : max_candidates) {
  const int N = params.horizon;
  check(cilqr_create(&params, max_candidates_, N, max_obstacles_, device_, &h_), "cilqr_create");
  control_seq_ = Matrix(params.num_ctrls, N);  // I/iLQR.cpp:9-15
  check(cilqr_default_control_seq(N, control_seq_.a.data()), "cilqr_default_control_seq");
}

iLQR::~iLQR() {
  if (noise_stream_) (void)hipStreamSynchronize((hipStream_t)noise_stream_);
  if (noise_dev_) (void)hipFree(noise_dev_);
  if (scov_dev_) (void)hipFree(scov_dev_);
  if (map_dev_) (void)hipFree(map_dev_);
  if (noise_stream_) (void)hipStreamDestroy((hipStream_t)noise_stream_);
  cilqr_destroy(h_);
}

void iLQR::set_Obstacle(const std::vector<Obstacle>& obstacles) {
  if ((int)obstacles.size() > max_obstacles_) throw std::runtime_error("set_Obstacle: more obstacles than max_obstacles");
  for (const Obstacle& o : obstacles)
    if (o.dimension.rows != 2 || o.relative_pos_array.rows != 4 || o.dimension.cols < params.horizon ||
        o.relative_pos_array.cols < params.horizon)
      throw std::runtime_error("set_Obstacle: dimension must be 2×horizon and relative_pos_array 4×horizon");
  if (tracked_horizon_ >= 0) obs_cov_.clear();  // (the covariance the prediction installed goes with its obstacles)
  tracked_horizon_ = -1;
  obstacles_ = obstacles;
  pack_obstacles();
}

void iLQR::clear_Obstacle() {
  if (tracked_horizon_ >= 0) obs_cov_.clear();
  tracked_horizon_ = -1;
  tracks_.clear(); track_dims_.clear(); track_cov_.clear(); track_Q_.clear();
  obstacles_.clear();
  pack_obstacles();
}

void iLQR::set_tracked_obstacles(const std::vector<double>& tracks, const std::vector<double>& dims, const std::vector<double>& cov,
                                 const std::vector<double>& Q) {
  const size_t M = tracks.size() / 6;
  if (tracks.size() != 6 * M || dims.size() != 2 * M || (!cov.empty() && cov.size() != 16 * M) || (!Q.empty() && Q.size() != 16))
    throw std::runtime_error("set_tracked_obstacles: needs 6 values per track, 2 dimensions, 16 covariance values or none, and 16 of Q or none");
  if ((int)M > max_obstacles_) throw std::runtime_error("set_tracked_obstacles: more tracks than max_obstacles");
  if (M == 0) { clear_Obstacle(); return; }
  tracks_ = tracks; track_dims_ = dims; track_cov_ = cov; track_Q_ = Q;
  install_tracked();
}

// The host form, in as few calls as the handle's arena allows: a call whose arrays do not fit is halved (a track's results depend on
// that track alone, so the split changes no bit).
void iLQR::install_tracked() {
  const int N = params.horizon, M = (int)(tracks_.size() / 6);
  std::vector<double> pose((size_t)M * 4 * N), dim((size_t)M * 2 * N), cov((size_t)M * 3 * N);
  int chunk = M;
  for (int m = 0; m < M;) {
    const int n = chunk < M - m ? chunk : M - m;
    const int rc = cilqr_predict_obstacles(h_, 1, N, n, &tracks_[(size_t)6 * m], &track_dims_[(size_t)2 * m],
                                           track_cov_.empty() ? nullptr : &track_cov_[(size_t)16 * m], track_Q_.empty() ? nullptr : track_Q_.data(),
                                           &pose[(size_t)m * 4 * N], &dim[(size_t)m * 2 * N], &cov[(size_t)m * 3 * N], nullptr);
    if (rc == CILQR_ERR_ARG && n > 1 && strstr(cilqr_last_error(), "does not fit")) { chunk = (n + 1) / 2; continue; }
    check(rc, "cilqr_predict_obstacles");
    m += n;
  }
  obstacles_.clear();
  for (int m = 0; m < M; ++m) {
    Matrix d(2, N), r(4, N);
    memcpy(d.a.data(), &dim[(size_t)m * 2 * N], (size_t)2 * N * sizeof(double));   // (column-major 2 x N is the table's [2N] row)
    memcpy(r.a.data(), &pose[(size_t)m * 4 * N], (size_t)4 * N * sizeof(double));
    obstacles_.emplace_back(params, d, r);
  }
  obs_cov_ = cov;
  tracked_horizon_ = N;
  pack_obstacles();
}

void iLQR::set_obstacle_covariance_check(bool on) {
  const bool was = obs_cov_check_;
  obs_cov_check_ = on;
  if (was != on && cov_check_) reserve_noise_buffers();
}

void iLQR::set_uncertainty_map(const Uncertainty& u) {
  if (u.layer.size() != (size_t)u.geom.rows * u.geom.cols) throw std::runtime_error("set_uncertainty_map: layer size does not match its geometry");
  apply_map(u);
  unc_ = u;  // (kept: set_map_tightening moves the layer between the handle's device copy and this object's)
  map_set_ = true;
}

namespace {
cilqr_uncertainty_map map_of(const Uncertainty& u, const float* layer, int64_t layer_stride) {
  cilqr_uncertainty_map m{};
  m.layer = layer;
  m.geom = u.geom;
  m.pose_x = u.pose_x; m.pose_y = u.pose_y; m.pose_theta = u.pose_theta;
  m.poses = nullptr;
  m.layer_stride = layer_stride;
  m.probes_l = u.probes_l; m.probes_w = u.probes_w;
  return m;
}
}  // namespace

// Without the map tightening: the host form, the handle keeps its own device copy.  With it: the layer is copied into map_dev_, in
// front of one tightened layer per candidate, and the handle is pointed there, so that the rounds can swap layers without a copy.
void iLQR::apply_map(const Uncertainty& u) {
  if (!map_in_block()) {
    const cilqr_uncertainty_map m = map_of(u, u.layer.data(), 0);
    check(cilqr_set_uncertainty_map(h_, &m), "cilqr_set_uncertainty_map");
    return;
  }
  // (with the track map beside the map tightening a round keeps two layers per candidate: the rasterised one and the tightened one)
  const size_t cells = (size_t)u.geom.rows * u.geom.cols, need = cells * (1 + (size_t)max_candidates_ * (map_tighten_ && tm_rounds_ > 0 ? 2 : 1));
  if (hipSetDevice(device_) != hipSuccess) throw std::runtime_error("set_uncertainty_map: hipSetDevice failed");
  if (noise_stream_) (void)hipStreamSynchronize((hipStream_t)noise_stream_);  // nothing enqueued may still read the old block
  if (need > map_dev_cap_) {
    if (map_dev_) (void)hipFree(map_dev_);
    map_dev_ = nullptr; map_dev_cap_ = 0;
    if (hipMalloc((void**)&map_dev_, need * sizeof(float)) != hipSuccess) throw std::runtime_error("set_uncertainty_map: hipMalloc failed");
    map_dev_cap_ = need;
  }
  if (hipMemcpy(map_dev_, u.layer.data(), cells * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    throw std::runtime_error("set_uncertainty_map: hipMemcpy failed");
  const cilqr_uncertainty_map m = map_of(u, map_dev_, 0);
  check(cilqr_set_uncertainty_map_device(h_, &m), "cilqr_set_uncertainty_map_device");
}

std::vector<double> iLQR::debug_map_cost(const std::vector<double>& states) const {
  const int n = (int)(states.size() / 4);
  std::vector<double> out((size_t)6 * n, 0.0);
  check(cilqr_debug_uncertainty_cost(h_, n, states.data(), out.data(), out.data() + n, out.data() + 3 * (size_t)n), "cilqr_debug_uncertainty_cost");
  return out;
}

cilqr_uncertainty_map iLQR::device_map(bool tightened) const {
  const int64_t cells = (int64_t)unc_.geom.rows * unc_.geom.cols;
  return tightened ? map_of(unc_, map_dev_ + cells, cells) : map_of(unc_, map_dev_, 0);
}

void iLQR::clear_uncertainty_map() {
  check(cilqr_clear_uncertainty_map(h_), "cilqr_clear_uncertainty_map");
  map_set_ = false;
}

void iLQR::set_global_plan(const Matrix& global_plan) {
  if (global_plan.rows != 2 || global_plan.cols < 1) throw std::runtime_error("set_global_plan: expected a 2×P matrix");
  global_plan_ = global_plan;
}

void iLQR::pack_obstacles() {
  // held: every column of every obstacle equals its first one, bit for bit (so that passing the first alone changes nothing)
  const int N = params.horizon;
  held_ = true;
  for (const Obstacle& o : obstacles_)
    for (int t = 1; t < N && held_; ++t)
      held_ = memcmp(&o.relative_pos_array.a[(size_t)4 * t], &o.relative_pos_array.a[0], 4 * sizeof(double)) == 0 &&
              memcmp(&o.dimension.a[(size_t)2 * t], &o.dimension.a[0], 2 * sizeof(double)) == 0;
  packed_horizon_ = N;
  const int M = (int)obstacles_.size();
  // a covariance per step needs an entry per step to sit beside (obs_cov shares the poses' entry index)
  if (M && N > 1 && obs_cov_.size() == (size_t)3 * M * N) held_ = false;
  const int T = held_ ? 1 : N;  // columns packed per obstacle
  obs_pose_.resize((size_t)M * 4 * T);
  obs_dim_.resize((size_t)M * 2 * T);
  for (int m = 0; m < M; ++m) {
    const Obstacle& o = obstacles_[m];
    for (int t = 0; t < T; ++t) {
      for (int r = 0; r < 4; ++r) obs_pose_[((size_t)m * T + t) * 4 + r] = o.relative_pos_array(r, t);
      for (int r = 0; r < 2; ++r) obs_dim_[((size_t)m * T + t) * 2 + r] = o.dimension(r, t);
    }
  }
  obs_cov_packed_.clear();
  if (M && (obs_cov_.size() == (size_t)3 * M || obs_cov_.size() == (size_t)3 * M * N)) {
    const bool per_step = obs_cov_.size() != (size_t)3 * M;
    obs_cov_packed_.resize((size_t)M * T * 3);
    for (int m = 0; m < M; ++m)
      for (int t = 0; t < T; ++t)
        for (int r = 0; r < 3; ++r) obs_cov_packed_[((size_t)m * T + t) * 3 + r] = obs_cov_[per_step ? ((size_t)m * N + t) * 3 + r : (size_t)m * 3 + r];
  }
}

cilqr_obstacles iLQR::obstacle_strides() {
  if (tracked_horizon_ >= 0 && tracked_horizon_ != params.horizon) install_tracked();  // (the horizon changed: predict again)
  if (packed_horizon_ != params.horizon) pack_obstacles();  // (params is public: the horizon may have changed since set_Obstacle)
  cilqr_obstacles o{};
  o.pose = obs_pose_.data();
  o.dim = obs_dim_.data();
  o.weight = nullptr;
  o.batch_stride = 0;
  o.obstacle_stride = held_ ? 1 : params.horizon;
  o.step_stride = held_ ? 0 : 1;
  o.weight_batch_stride = 0;
  return o;
}

void iLQR::get_optimal_control_seq(const double x_0[4], Matrix& U, const double poly_coeffs[6],
                                   const std::vector<double>& x_local_plan) {
  if (tracked_horizon_ >= 0 && tracked_horizon_ != params.horizon) install_tracked();
  const int N = params.horizon, M = (int)obstacles_.size();
  if (U.rows != 2 || U.cols != N) throw std::runtime_error("get_optimal_control_seq: U must be 2×horizon");
  if (x_local_plan.empty()) throw std::runtime_error("get_optimal_control_seq: empty x_local_plan");
  const double fl[2] = {x_local_plan.front(), x_local_plan.back()};
  if (tighten_ || map_tighten_ || track_map_on()) { solve_tightened(x_0, U, poly_coeffs, fl); return; }
  X_result = Matrix(4, N + 1);
  int32_t iters = 0, status = 0;
  if (n_samples_) {
    std::vector<double> pose, dim, off;
    const int n_obs = pack_sampled(1, pose, dim, off);
    check(cilqr_solve_batch_sampled(h_, 1, N, n_obs, n_samples_, x_0, U.a.data(), poly_coeffs, fl, pose.data(), dim.data(), off.data(),
                                    sample_weight(), X_result.a.data(), &last_cost, &iters, &status, CILQR_FLAG_NONE),
          "cilqr_solve_batch_sampled");
    last_iterations = iters;
    last_exit = status;
    U_result = U;
    return;
  }
  const cilqr_obstacles obs = obstacle_strides();
  check(cilqr_solve_batch_obstacles(h_, 1, N, M, x_0, U.a.data(), poly_coeffs, fl, M ? &obs : nullptr, X_result.a.data(), &last_cost,
                                    &iters, &status, CILQR_FLAG_NONE),
        "cilqr_solve_batch_obstacles");
  last_iterations = iters;
  last_exit = status;
  U_result = U;  // I/iLQR.cpp:244
}

void iLQR::run_step(const double ego_state[4]) {
  if (global_plan_.cols < 1) throw std::runtime_error("run_step: set_global_plan was not called");
  double coeffs[CILQR_POLY_COEFFS];
  std::vector<double> ref(2 * (size_t)params.num_of_local_wpts);
  int n = 0;
  check(cilqr_local_plan(&params, global_plan_.a.data(), global_plan_.cols, ego_state, coeffs, ref.data(), &n), "cilqr_local_plan");
  std::vector<double> x_local_plan(n);
  ref_traj_result = Matrix(2, n);
  for (int i = 0; i < n; ++i) {
    x_local_plan[i] = ref[2 * i];
    ref_traj_result(0, i) = ref[2 * i];
    ref_traj_result(1, i) = ref[2 * i + 1];
  }
  get_optimal_control_seq(ego_state, control_seq_, coeffs, x_local_plan);  // I/iLQR.cpp:253: warm start persists
}

Experiment flatten_experiment(const double start_pos[4], double planning_time, const Matrix& X, const Matrix& U) {
  Experiment e;
  e.planning_time = planning_time;
  e.start_pos.assign(start_pos, start_pos + 4);
  e.X.resize(4 * (size_t)(U.cols + 1));
  e.U.resize(2 * (size_t)U.cols);
  for (int i = 0; i < U.cols + 1; ++i)
    for (int r = 0; r < 4; ++r) e.X[4 * i + r] = X(r, i);
  for (int i = 0; i < U.cols; ++i)
    for (int r = 0; r < 2; ++r) e.U[2 * i + r] = U(r, i);
  return e;
}

void iLQR::set_candidate_pick(CandidatePick pick, double max_collision) {
  pick_ = pick;
  max_collision_ = max_collision;
}

int iLQR::run_candidates(const std::vector<double>& ego_states) {
  if (tracked_horizon_ >= 0 && tracked_horizon_ != params.horizon) install_tracked();
  const int B = (int)(ego_states.size() / 4), N = params.horizon, M = (int)obstacles_.size();
  if (B < 1 || B > max_candidates_) throw std::runtime_error("run_candidates: candidate count outside [1, max_candidates]");
  if (global_plan_.cols < 1) throw std::runtime_error("run_candidates: set_global_plan was not called");
  if (scov_check_ && track_map_on())
    throw std::logic_error("set_track_map has no form for sampled obstacles (set_obstacle_samples), like set_map_tightening");
  if (scov_check_) return run_candidates_sample_covariance(B, ego_states);
  if (!noise_.empty() || cov_check_ || tighten_ || map_tighten_ || track_map_on()) return run_candidates_noise_checked(B, ego_states);
  std::vector<double> U((size_t)B * 2 * N), poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2);
  std::vector<double> X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B);
  // LocalPlanner pre-step for all candidates in one device launch (cilqr_local_plan_batch) instead of B host fits
  const int W = params.num_of_local_wpts;
  std::vector<double> ref((size_t)B * 2 * W);
  std::vector<int32_t> n_ref(B);
  check(cilqr_local_plan_batch(h_, B, global_plan_.cols, global_plan_.a.data(), 0, ego_states.data(), poly.data(), fl.data(),
                               ref.data(), n_ref.data()), "cilqr_local_plan_batch");
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 2 * N; ++i) U[(size_t)b * 2 * N + i] = control_seq_.a[i];
  const cilqr_obstacles obs = obstacle_strides();  // one obstacle set for every candidate
  std::vector<double> total, nom_pose, nom_dim, samp_off;
  const int n_obs = n_samples_ ? pack_sampled(B, nom_pose, nom_dim, samp_off) : 0;
  if (n_samples_)
    check(cilqr_solve_batch_sampled(h_, B, N, n_obs, n_samples_, ego_states.data(), U.data(), poly.data(), fl.data(), nom_pose.data(),
                                    nom_dim.data(), samp_off.data(), sample_weight(), X.data(), J.data(), iters.data(), status.data(),
                                    CILQR_FLAG_NONE),
          "cilqr_solve_batch_sampled");
  else
    check(cilqr_solve_batch_obstacles(h_, B, N, M, ego_states.data(), U.data(), poly.data(), fl.data(), M ? &obs : nullptr, X.data(),
                                      J.data(), iters.data(), status.data(), CILQR_FLAG_NONE),
          "cilqr_solve_batch_obstacles");
  last_scores.clear();
  if (pick_ == CandidatePick::MinTotalCost) {  // rank by everything the solve descended along, among the candidates that are safe
    last_scores.resize((size_t)B * CILQR_SCORE_FIELDS);
    total.resize(B);
    if (n_samples_)
      check(cilqr_score_batch_sampled(h_, B, N, n_obs, n_samples_, X.data(), U.data(), poly.data(), fl.data(), nom_pose.data(),
                                      nom_dim.data(), samp_off.data(), sample_weight(), max_collision_, last_scores.data(), total.data()),
            "cilqr_score_batch_sampled");
    else
      check(cilqr_score_batch(h_, B, N, M, X.data(), U.data(), poly.data(), fl.data(), M ? &obs : nullptr, max_collision_,
                              last_scores.data(), total.data()),
            "cilqr_score_batch");
  }
  const std::vector<double>& rank = pick_ == CandidatePick::MinTotalCost ? total : J;
  int best = 0;  // strict-< first minimum, NaN never wins (the convention of cilqr_argmin_device)
  bool have = false;
  for (int b = 0; b < B; ++b)
    if (rank[b] == rank[b] && (!have || rank[b] < rank[best])) { best = b; have = true; }
  if (pick_ == CandidatePick::MinTotalCost && !have) return -1;  // every candidate rejected: results and warm start stay
  X_result = Matrix(4, N + 1);
  for (int i = 0; i < 4 * (N + 1); ++i) X_result.a[i] = X[(size_t)best * 4 * (N + 1) + i];
  for (int i = 0; i < 2 * N; ++i) control_seq_.a[i] = U[(size_t)best * 2 * N + i];
  U_result = control_seq_;
  ref_traj_result = Matrix(2, n_ref[best]);
  for (int i = 0; i < 2 * n_ref[best]; ++i) ref_traj_result.a[i] = ref[(size_t)best * 2 * W + i];
  last_iterations = iters[best];
  last_exit = status[best];
  last_cost = J[best];
  return best;
}

namespace {
void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

namespace {
const char* const kObstacleCovarianceSize =
    "set_obstacle_covariance: needs 3 values per obstacle of set_Obstacle, or 3 per obstacle and step";
const char* const kStoredRowsWithSamples =
    "the stored-rows pose-noise check has no form for sampled obstacles (set_obstacle_samples): use set_pose_noise_check_fused";
const char* const kCovarianceWithNoise =
    "set_pose_covariance_check and set_pose_noise_check(_fused) are both set: the pose noise is given either as a covariance or as draws";
const char* const kTighteningWithSamples =
    "set_chance_tightening has no form for sampled obstacles (set_obstacle_samples): the sampled solve takes no inflated table";
const char* const kMapTighteningWithSamples =
    "set_map_tightening has no form for sampled obstacles (set_obstacle_samples), like set_chance_tightening";
const char* const kTighteningsDisagree =
    "set_chance_tightening and set_map_tightening are both set and must agree on Sigma0, W, lamb and rounds: one covariance chain and one "
    "re-solve per round serve both";
const char* const kTrackMapWithSamples =
    "set_track_map has no form for sampled obstacles (set_obstacle_samples), like set_map_tightening";
const char* const kTrackMapRoundsDisagree =
    "set_track_map beside set_chance_tightening or set_map_tightening: one re-solve per round serves them all, so the round counts must agree";
const char* const kTrackMapEllipsesOffTightened =
    "set_track_map with ellipses = false beside set_chance_tightening: the solves read no ellipse that the tightening could inflate";
const char* const kCovarianceWithSamples =
    "set_pose_covariance_check has no form for sampled obstacles (set_obstacle_samples): use set_sample_covariance_check";
const char* const kSampleCovarianceWithNoise =
    "set_sample_covariance_check and set_pose_noise_check(_fused) are both set: the pose noise is given either as a covariance or as draws";
const char* const kSampleCovarianceWithoutSamples =
    "set_sample_covariance_check has effect with obstacle samples (set_obstacle_samples) only: without samples use set_pose_covariance_check";
}  // namespace

void iLQR::set_obstacle_samples(const std::vector<double>& offsets, int n_samples) {
  if (offsets.empty()) {
    samples_.clear();
    n_samples_ = 0;
  } else {
    if (n_samples < 2 || offsets.size() % ((size_t)3 * n_samples) != 0)
      throw std::runtime_error("set_obstacle_samples: needs n_samples >= 2 and n_obs * n_samples * 3 offsets");
    if (offsets.size() / 3 > (size_t)max_obstacles_) throw std::runtime_error("set_obstacle_samples: n_obs * n_samples above max_obstacles");
    if (cov_check_) throw std::logic_error(kCovarianceWithSamples);
    if (tighten_) throw std::logic_error(kTighteningWithSamples);
    if (map_tighten_) throw std::logic_error(kMapTighteningWithSamples);
    samples_ = offsets;
    n_samples_ = n_samples;
  }
  last_risk.clear();
  last_step_hits.clear();
  if (!noise_.empty() || cov_check_ || rounds_on()) reserve_noise_buffers();  // (the device block holds other arrays with samples than without)
}

int iLQR::pack_sampled(int B, std::vector<double>& pose, std::vector<double>& dim, std::vector<double>& off) const {
  const size_t N = params.horizon, n_obs = obstacles_.size(), ns = n_samples_;
  if (n_obs < 1 || n_obs * ns * 3 != samples_.size())
    throw std::runtime_error("set_obstacle_samples: the offsets do not match the obstacles of set_Obstacle (n_obs * n_samples * 3)");
  for (const Obstacle& o : obstacles_)
    if ((size_t)o.dimension.cols < N || (size_t)o.relative_pos_array.cols < N)
      throw std::runtime_error("set_Obstacle: dimension must be 2×horizon and relative_pos_array 4×horizon");
  pose.resize((size_t)B * n_obs * 4 * N);
  dim.resize((size_t)B * n_obs * 2 * N);
  off.resize((size_t)B * samples_.size());
  for (size_t m = 0; m < n_obs; ++m) {
    const Obstacle& o = obstacles_[m];
    for (size_t t = 0; t < N; ++t) {
      for (int r = 0; r < 4; ++r) pose[(m * N + t) * 4 + r] = o.relative_pos_array(r, (int)t);
      for (int r = 0; r < 2; ++r) dim[(m * N + t) * 2 + r] = o.dimension(r, (int)t);
    }
  }
  for (int b = 1; b < B; ++b) {
    memcpy(&pose[(size_t)b * n_obs * 4 * N], pose.data(), n_obs * 4 * N * sizeof(double));
    memcpy(&dim[(size_t)b * n_obs * 2 * N], dim.data(), n_obs * 2 * N * sizeof(double));
  }
  for (int b = 0; b < B; ++b) memcpy(&off[(size_t)b * samples_.size()], samples_.data(), samples_.size() * sizeof(double));
  return (int)n_obs;
}

void iLQR::set_pose_noise_check(const std::vector<double>& offsets, double max_risk, double lamb) {
  if (offsets.size() % 4 != 0) throw std::runtime_error("set_pose_noise_check: offsets must hold 4 doubles per sample");
  if (n_samples_ && !offsets.empty()) throw std::logic_error(kStoredRowsWithSamples);
  if (cov_check_ && !offsets.empty()) throw std::logic_error(kCovarianceWithNoise);
  if (scov_check_ && !offsets.empty()) throw std::logic_error(kSampleCovarianceWithNoise);
  noise_ = offsets;
  max_risk_ = max_risk;
  noise_lamb_ = lamb;
  noise_fused_ = false;
  last_risk.clear();
  last_step_hits.clear();
  if (!noise_.empty() || rounds_on()) reserve_noise_buffers();
}

void iLQR::set_pose_noise_check_fused(const std::vector<double>& offsets, double max_risk, double lamb) {
  if (offsets.size() % 4 != 0) throw std::runtime_error("set_pose_noise_check_fused: offsets must hold 4 doubles per sample");
  if (cov_check_ && !offsets.empty()) throw std::logic_error(kCovarianceWithNoise);
  if (scov_check_ && !offsets.empty()) throw std::logic_error(kSampleCovarianceWithNoise);
  noise_ = offsets;
  max_risk_ = max_risk;
  noise_lamb_ = lamb;
  noise_fused_ = true;
  last_risk.clear();
  last_step_hits.clear();
  if (!noise_.empty() || rounds_on()) reserve_noise_buffers();
}

void iLQR::set_map_risk_check(double occ_threshold, double max_risk, bool unknown_hits) {
  if (max_risk != max_risk) throw std::runtime_error("set_map_risk_check: max_risk is NaN");
  map_check_ = occ_threshold == occ_threshold;  // NaN: off
  map_threshold_ = occ_threshold;
  map_max_risk_ = max_risk;
  map_unknown_hits_ = unknown_hits;
  last_map_risk.clear();
  last_map_step_hits.clear();
  last_map_unknown_hits.clear();
}

void iLQR::set_pose_covariance_check(const double Sigma0[16], const double* W, double max_risk, double lamb, bool sum_bound) {
  if (Sigma0 && !noise_.empty()) throw std::logic_error(kCovarianceWithNoise);
  if (Sigma0 && n_samples_) throw std::logic_error(kCovarianceWithSamples);
  if (max_risk != max_risk) throw std::runtime_error("set_pose_covariance_check: max_risk is NaN");
  cov_check_ = Sigma0 != nullptr;
  cov_has_W_ = cov_check_ && W != nullptr;
  if (cov_check_) memcpy(cov_sigma0_, Sigma0, sizeof(cov_sigma0_));
  if (cov_has_W_) memcpy(cov_W_, W, sizeof(cov_W_));
  cov_max_risk_ = max_risk;
  cov_lamb_ = lamb;
  cov_sum_ = sum_bound;
  last_chance_risk.clear();
  last_step_risk.clear();
  if (cov_check_ || rounds_on()) reserve_noise_buffers();
}

void iLQR::set_sample_covariance_check(const double Sigma0[16], const double* W, double max_risk, double lamb, bool sum_bound) {
  if (Sigma0 && !noise_.empty()) throw std::logic_error(kSampleCovarianceWithNoise);
  if (max_risk != max_risk) throw std::runtime_error("set_sample_covariance_check: max_risk is NaN");
  scov_check_ = Sigma0 != nullptr;
  scov_has_W_ = scov_check_ && W != nullptr;
  if (scov_check_) memcpy(scov_sigma0_, Sigma0, sizeof(scov_sigma0_));
  if (scov_has_W_) memcpy(scov_W_, W, sizeof(scov_W_));
  scov_max_risk_ = max_risk;
  scov_lamb_ = lamb;
  scov_sum_ = sum_bound;
  last_chance_risk_sampled.clear();
}

void iLQR::set_map_covariance_check(double occ_threshold, double max_risk, int nx, int ny, int nth, bool sum_bound, bool unknown_hits) {
  if (max_risk != max_risk) throw std::runtime_error("set_map_covariance_check: max_risk is NaN");
  const bool on = occ_threshold == occ_threshold;  // NaN: off
  std::vector<double> nodes, weights;
  if (on) {  // the nodes are built here, once
    if (nx < 1 || ny < 1 || nth < 1 || nx > 9 || ny > 9 || nth > 9) throw std::runtime_error("set_map_covariance_check: 1 ... 9 nodes per axis");
    nodes.assign((size_t)nx * ny * nth * 3, 0.0);
    weights.assign((size_t)nx * ny * nth, 0.0);
    check(cilqr_pose_quadrature(nx, ny, nth, nodes.data(), weights.data()), "cilqr_pose_quadrature");
    if (weights.size() > CILQR_MAX_QUAD_NODES) throw std::runtime_error("set_map_covariance_check: more than CILQR_MAX_QUAD_NODES nodes");
  }
  cmap_check_ = on;
  cmap_nodes_ = nodes;
  cmap_weights_ = weights;
  cmap_threshold_ = occ_threshold;
  cmap_max_risk_ = max_risk;
  cmap_sum_ = sum_bound;
  cmap_unknown_hits_ = unknown_hits;
  last_chance_map_risk.clear();
  last_map_step_risk.clear();
  if (cov_check_) reserve_noise_buffers();  // (the device block holds Sigma_t and the nodes while this check is on)
}

void iLQR::set_chance_tightening(const double Sigma0[16], const double* W, double eps, int rounds, double max_inflate, double lamb) {
  const bool on = Sigma0 != nullptr && rounds != 0;
  if (on && n_samples_) throw std::logic_error(kTighteningWithSamples);
  if (on && rounds < 0) throw std::runtime_error("set_chance_tightening: rounds is negative");
  const double kappa = on ? cilqr_chance_kappa(eps) : 0.0;
  if (kappa != kappa) throw std::runtime_error("set_chance_tightening: eps outside (0, 0.5]");
  if (on && !(max_inflate >= 0.0 && max_inflate <= 1.7e308)) throw std::runtime_error("set_chance_tightening: max_inflate is negative or not finite");
  if (on) check_tightening_agrees(map_tighten_, mt_rounds_, Sigma0, W, lamb, rounds);
  tighten_ = on;
  if (on) {  // (Sigma0, W and lamb are the one set both tightenings read; switched off, a map tightening keeps them as they are)
    tg_has_W_ = W != nullptr;
    memcpy(tg_sigma0_, Sigma0, sizeof(tg_sigma0_));
    if (tg_has_W_) memcpy(tg_W_, W, sizeof(tg_W_));
    tg_lamb_ = lamb;
  } else if (!map_tighten_) {
    tg_has_W_ = false;
  }
  tg_kappa_ = kappa;
  tg_rounds_ = on ? rounds : 0;
  tg_cap_ = max_inflate;
  last_tighten.clear();
  last_tighten_risk_before.clear();
  if (rounds_on()) reserve_noise_buffers();
}

void iLQR::check_tightening_agrees(bool other_on, int other_rounds, const double Sigma0[16], const double* W, double lamb, int rounds) const {
  if (!other_on) return;
  const bool same = memcmp(tg_sigma0_, Sigma0, sizeof(tg_sigma0_)) == 0 && tg_has_W_ == (W != nullptr) &&
                    (!tg_has_W_ || memcmp(tg_W_, W, sizeof(tg_W_)) == 0) && tg_lamb_ == lamb && other_rounds == rounds;
  if (!same) throw std::logic_error(kTighteningsDisagree);
}

void iLQR::set_map_tightening(const double Sigma0[16], const double* W, double eps, int rounds, double max_inflate, double lamb) {
  const bool on = Sigma0 != nullptr && rounds != 0;
  if (on && n_samples_) throw std::logic_error(kMapTighteningWithSamples);
  if (on && rounds < 0) throw std::runtime_error("set_map_tightening: rounds is negative");
  const double kappa = on ? cilqr_chance_kappa(eps) : 0.0;
  if (kappa != kappa) throw std::runtime_error("set_map_tightening: eps outside (0, 0.5]");
  if (on && !(max_inflate >= 0.0 && max_inflate <= 1.7e308)) throw std::runtime_error("set_map_tightening: max_inflate is negative or not finite");
  if (on) check_tightening_agrees(tighten_, tg_rounds_, Sigma0, W, lamb, rounds);
  const bool was = map_tighten_;
  map_tighten_ = on;
  if (on) {  // (Sigma0, W and lamb are the one set both tightenings read)
    tg_has_W_ = W != nullptr;
    memcpy(tg_sigma0_, Sigma0, sizeof(tg_sigma0_));
    if (tg_has_W_) memcpy(tg_W_, W, sizeof(tg_W_));
    tg_lamb_ = lamb;
  }
  mt_kappa_ = kappa;
  mt_rounds_ = on ? rounds : 0;
  mt_cap_ = max_inflate;
  last_tighten_map.clear();
  last_tighten_map_risk_before.clear();
  if (map_set_ && (was != on || map_in_block())) apply_map(unc_);  // the layer moves to this object's device block, or back to the handle's
  if (rounds_on()) reserve_noise_buffers();
}

void iLQR::set_track_map(double inflate, double z_max, int window, int rounds, bool ellipses) {
  if (rounds < 0 || window < 0 || !(inflate >= 0.0 && inflate <= 1.7e308) || !(z_max >= 0.0 && z_max <= 1.7e308))
    throw std::runtime_error("set_track_map: rounds and window must not be negative, inflate and z_max neither negative nor not finite");
  const bool was = map_in_block();
  tm_rounds_ = rounds; tm_window_ = window; tm_inflate_ = inflate; tm_z_max_ = z_max; tm_ellipses_ = ellipses;
  last_track_map.clear();
  if (map_set_ && (was != map_in_block() || map_in_block())) apply_map(unc_);  // the layer moves to this object's device block, or back
  if (rounds_on()) reserve_noise_buffers();
}

// Before anything is enqueued: what a run under set_track_map cannot be combined with.
void iLQR::check_track_map_conflicts() const {
  if (!track_map_on()) return;
  if (n_samples_) throw std::logic_error(kTrackMapWithSamples);
  const bool obs_on = tighten_ && !obstacles_.empty(), map_on = map_tightened();
  if (obs_on && !tm_ellipses_) throw std::logic_error(kTrackMapEllipsesOffTightened);
  if ((obs_on && tg_rounds_ != tm_rounds_) || (map_on && mt_rounds_ != tm_rounds_)) throw std::logic_error(kTrackMapRoundsDisagree);
}

void iLQR::set_obstacle_covariance(const std::vector<double>& cov) {
  obs_cov_ = cov;
  pack_obstacles();
}

// One device block for max_candidates candidates x S rollouts at the current horizon; the offsets travel here, once.  The fused
// check stores no rollout rows: it keeps the nominal score rows, their totals and the step counts instead.
void iLQR::reserve_noise_buffers() {
  // (the covariance check has no draws: it keeps ONE zero offset, the plan itself, for the map risk call, and the fused check's arrays)
  // (tightening alone, with no check behind it, keeps the fused check's score rows and totals for a MinTotalCost pick)
  const bool fused = noise_fused_ || cov_check_ || noise_.empty();
  const size_t B = max_candidates_, S = cov_check_ ? 1 : noise_.size() / 4, N = params.horizon, M = max_obstacles_, R = fused ? 0 : B * S;
  // with obstacle samples: per-candidate nominal tables and offsets in place of the one shared set (n_obs * n_samples <= M)
  const size_t n_obs = n_samples_ ? samples_.size() / 3 / n_samples_ : 0;
  size_t o = 0;
  const auto take = [&o](size_t doubles) { const size_t at = o; o += (doubles + 1) & ~(size_t)1; return at; };
  NoiseLayout& L = nl_;
  L.x0 = take(B * 4); L.U = take(B * 2 * N); L.poly = take(B * CILQR_POLY_COEFFS); L.fl = take(B * 2);
  L.pose = take(n_samples_ ? B * n_obs * 4 * N : M * 4 * N); L.dim = take(n_samples_ ? B * n_obs * 2 * N : M * 2 * N);
  L.soff = take(B * samples_.size());
  L.X = take(B * 4 * (N + 1)); L.J = take(B); L.iters = take(B); L.status = take(B);
  L.k = take(B * 2 * N); L.K = take(B * 8 * N); L.ok = take(B);
  L.delta = take(S * 4);
  L.Xr = take(R * 4 * (N + 1)); L.Ur = take(R * 2 * N); L.rows = take(R * CILQR_SCORE_FIELDS);
  L.risk = take(B * (n_samples_ ? CILQR_RRS_FIELDS : fused ? CILQR_ROLLOUT_RISK_FIELDS : CILQR_RISK_FIELDS)); L.total = take(B); L.pair = take(2);
  L.score = take(fused ? B * CILQR_SCORE_FIELDS : 0); L.base = take(fused ? B : 0); L.hits = take(fused ? (B * N + 1) / 2 : 0);
  // the map risk check's outputs (a few doubles per candidate: reserved with the fused check whether or not the check is on)
  L.mrisk = take(fused ? B * CILQR_MAP_RISK_FIELDS : 0); L.mtotal = take(fused ? B : 0);
  L.mhits = take(fused ? (B * N + 1) / 2 : 0); L.munk = take(fused ? (B * N + 1) / 2 : 0);
  // the covariance check's inputs and outputs
  L.s0 = take(cov_check_ ? 16 : 0); L.W = take(cov_check_ ? 16 : 0);
  L.crisk = take(cov_check_ ? B * CILQR_CHANCE_FIELDS : 0); L.cstep = take(cov_check_ ? B * N : 0);
  L.ccov = take(cov_check_ && obs_cov_check_ ? M * N * 3 : 0);  // the obstacles' covariance for the judge (set_obstacle_covariance_check)
  // the map covariance check: every Sigma_t of the chance call, the nodes and weights, its outputs
  const size_t cm = cov_check_ && cmap_check_ ? 1 : 0, Q = cmap_weights_.size();
  L.csig = take(cm * B * (N + 1) * 16); L.qn = take(cm * Q * 3); L.qw = take(cm * Q);
  L.cmrisk = take(cm * B * CILQR_CHANCE_MAP_FIELDS); L.cmstep = take(cm * B * N); L.cmtotal = take(cm * B);
  // the tightening rounds: Sigma0, W, every Sigma_t, the risk row of the round's input plan, the inflated dense table, the fields, obs_cov
  // (the map tightening shares the chain's arrays and adds its fields; its layers are floats and lie in map_dev_)
  const size_t tg = tighten_ ? 1 : 0, chain = tighten_ || map_tighten_ ? 1 : 0;
  L.ts0 = take(chain * 16); L.tW = take(chain * 16); L.tsig = take(chain * B * (N + 1) * 16); L.trisk = take(chain * B * CILQR_CHANCE_FIELDS);
  L.tpose = take(tg * B * M * 4 * N); L.tdim = take(tg * B * M * 2 * N); L.tg = take(tg * B * CILQR_TIGHTEN_FIELDS); L.tcov = take(tg * M * N * 3);
  L.tmg = take((map_tighten_ ? 1 : 0) * B * CILQR_TIGHTEN_MAP_FIELDS);
  // the track map's rounds: the tracks' covariance by the packed obstacles' strides, the fields
  L.tkcov = take((tm_rounds_ > 0 ? 1 : 0) * M * N * 3); L.tkf = take((tm_rounds_ > 0 ? 1 : 0) * B * CILQR_TRACK_MAP_FIELDS);
  L.end = o;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  if (!noise_stream_) {
    hipStream_t st;
    hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreateWithFlags");
    noise_stream_ = st;
  }
  hip_check(hipStreamSynchronize((hipStream_t)noise_stream_), "hipStreamSynchronize");
  if (noise_dev_) hip_check(hipFree(noise_dev_), "hipFree");
  noise_dev_ = nullptr;
  hip_check(hipMalloc(&noise_dev_, L.end * sizeof(double)), "hipMalloc");
  if (cov_check_) hip_check(hipMemset((double*)noise_dev_ + L.delta, 0, 4 * sizeof(double)), "hipMemset");
  else if (!noise_.empty()) hip_check(hipMemcpy((double*)noise_dev_ + L.delta, noise_.data(), noise_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  if (cm) {
    hip_check(hipMemcpy((double*)noise_dev_ + L.qn, cmap_nodes_.data(), cmap_nodes_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy((double*)noise_dev_ + L.qw, cmap_weights_.data(), cmap_weights_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  }
  noise_horizon_ = params.horizon;
}

int iLQR::run_candidates_noise_checked(int B, const std::vector<double>& ego_states) {
  const int N = params.horizon, M = (int)obstacles_.size(), S = cov_check_ ? 1 : (int)(noise_.size() / 4);
  if (cov_check_ && !noise_.empty()) throw std::logic_error(kCovarianceWithNoise);
  if (cov_check_ && n_samples_) throw std::logic_error(kCovarianceWithSamples);
  if (tighten_ && n_samples_) throw std::logic_error(kTighteningWithSamples);
  if (map_tighten_ && n_samples_) throw std::logic_error(kMapTighteningWithSamples);
  if (n_samples_ && !noise_fused_) throw std::logic_error(kStoredRowsWithSamples);
  check_track_map_conflicts();
  if (noise_horizon_ != N) reserve_noise_buffers();  // (params is public: the horizon may have changed since the setter)
  std::vector<double> U((size_t)B * 2 * N), poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2);
  const int W = params.num_of_local_wpts;
  std::vector<double> ref((size_t)B * 2 * W);
  std::vector<int32_t> n_ref(B);
  check(cilqr_local_plan_batch(h_, B, global_plan_.cols, global_plan_.a.data(), 0, ego_states.data(), poly.data(), fl.data(),
                               ref.data(), n_ref.data()), "cilqr_local_plan_batch");
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 2 * N; ++i) U[(size_t)b * 2 * N + i] = control_seq_.a[i];
  const cilqr_obstacles host_obs = obstacle_strides();
  if ((tighten_ || (cov_check_ && obs_cov_check_)) && M && !obs_cov_.empty() && obs_cov_packed_.empty()) throw std::runtime_error(kObstacleCovarianceSize);
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hipStream_t st = (hipStream_t)noise_stream_;
  double* d = (double*)noise_dev_;
  const NoiseLayout& L = nl_;
  const auto up = [&](size_t at, const void* src, size_t doubles) {
    if (doubles) hip_check(hipMemcpyAsync(d + at, src, doubles * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  };
  const auto down = [&](void* dst, size_t at, size_t bytes) {
    hip_check(hipMemcpyAsync(dst, d + at, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  };
  up(L.x0, ego_states.data(), (size_t)B * 4);
  up(L.U, U.data(), U.size());
  up(L.poly, poly.data(), poly.size());
  up(L.fl, fl.data(), fl.size());
  std::vector<double> nom_pose, nom_dim, samp_off;  // (alive until the stream has been waited for)
  const int n_obs = n_samples_ ? pack_sampled(B, nom_pose, nom_dim, samp_off) : 0;
  if (n_samples_) {
    up(L.pose, nom_pose.data(), nom_pose.size());
    up(L.dim, nom_dim.data(), nom_dim.size());
    up(L.soff, samp_off.data(), samp_off.size());
  } else {
    up(L.pose, obs_pose_.data(), obs_pose_.size());
    up(L.dim, obs_dim_.data(), obs_dim_.size());
  }
  cilqr_obstacles obs = host_obs;  // the same strides over the device copies
  obs.pose = d + L.pose;
  obs.dim = d + L.dim;
  const cilqr_obstacles* po = M ? &obs : nullptr;
  // under set_track_map with ellipses off the SOLVES read no ellipse: the tracks reach them through the map only; every check still sees them
  const int Ms = track_map_on() && !tm_ellipses_ ? 0 : M;
  const cilqr_obstacles* pos = Ms ? po : nullptr;
  const int risk_fields = n_samples_ ? CILQR_RRS_FIELDS : noise_fused_ ? CILQR_ROLLOUT_RISK_FIELDS : CILQR_RISK_FIELDS;
  int rc = CILQR_OK;
  const bool plain = !cov_check_ && noise_.empty();  // tightening alone: no check behind it, the pick of run_candidates itself
  const bool scored = cov_check_ || plain ? pick_ == CandidatePick::MinTotalCost : noise_fused_;  // last_scores is filled
  const bool obs_tightened = tighten_ && M > 0, tightened = obs_tightened || map_tightened() || track_map_on();
  const bool cmap_checked = cmap_check_ && map_set_ && cov_check_;
  if (plain) {
    rc = cilqr_solve_batch_obstacles_device(h_, st, B, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, pos, d + L.X, d + L.J,
                                            (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
    if (!rc && tightened) rc = tighten_rounds(st, d, B, po);
    if (!rc && scored) rc = cilqr_score_batch_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, max_collision_, d + L.score, d + L.total);
  } else if (cov_check_) {  // the analytic check: covariance chain and chance values in place of rollouts
    up(L.s0, cov_sigma0_, 16);
    if (cov_has_W_) up(L.W, cov_W_, 16);
    rc = cilqr_solve_batch_obstacles_device(h_, st, B, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, pos, d + L.X, d + L.J,
                                            (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
    if (!rc && tightened) rc = tighten_rounds(st, d, B, po);
    if (!rc && scored) rc = cilqr_score_batch_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, 1.0, d + L.score, d + L.base);
    if (!rc) rc = cilqr_gains_batch_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, cov_lamb_, d + L.k, d + L.K, (int32_t*)(d + L.ok));
    // (the judge counts the obstacles' own covariance when asked to and one is set; its entries lie by the packed obstacles' strides)
    const bool judge_cov = obs_cov_check_ && M > 0 && !obs_cov_packed_.empty();
    if (judge_cov) up(L.ccov, obs_cov_packed_.data(), obs_cov_packed_.size());
    if (!rc && judge_cov)
      rc = cilqr_chance_risk_cov_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.K, d + L.s0, 0, cov_has_W_ ? d + L.W : nullptr, po, d + L.ccov,
                                        cov_sum_ ? CILQR_CHANCE_BOUND_SUM : 0u, cov_max_risk_, d + (scored ? L.base : L.J), d + L.crisk,
                                        d + L.cstep, nullptr, cmap_checked ? d + L.csig : nullptr, d + L.total);
    else if (!rc)
      rc = cilqr_chance_risk_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.K, d + L.s0, 0, cov_has_W_ ? d + L.W : nullptr, po,
                                    cov_sum_ ? CILQR_CHANCE_BOUND_SUM : 0u, cov_max_risk_, d + (scored ? L.base : L.J), d + L.crisk,
                                    d + L.cstep, nullptr, cmap_checked ? d + L.csig : nullptr, d + L.total);
  } else if (n_samples_) {  // the same chain in the compact sampled form
    const int ns = n_samples_;
    const double w = sample_weight();
    rc = cilqr_solve_batch_sampled_device(h_, st, B, N, n_obs, ns, d + L.x0, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim, d + L.soff, w,
                                          d + L.X, d + L.J, (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
    if (!rc) rc = cilqr_gains_batch_sampled_device(h_, st, B, N, n_obs, ns, d + L.X, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                   d + L.soff, w, noise_lamb_, d + L.k, d + L.K, (int32_t*)(d + L.ok));
    if (!rc) rc = cilqr_score_batch_sampled_device(h_, st, B, N, n_obs, ns, d + L.X, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                   d + L.soff, w, 1.0, d + L.score, d + L.base);
    if (!rc) rc = cilqr_rollout_risk_sampled_device(h_, st, B, N, n_obs, ns, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0,
                                                    d + L.pose, d + L.dim, d + L.soff, max_risk_, d + L.base, d + L.risk,
                                                    (int32_t*)(d + L.hits), d + L.total);
  } else {
    rc = cilqr_solve_batch_obstacles_device(h_, st, B, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, pos, d + L.X, d + L.J,
                                            (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
    if (!rc && tightened) rc = tighten_rounds(st, d, B, po);
    if (!rc) rc = cilqr_gains_batch_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, noise_lamb_, d + L.k, d + L.K, (int32_t*)(d + L.ok));
    if (noise_fused_) {
      if (!rc) rc = cilqr_score_batch_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, 1.0, d + L.score, d + L.base);
      if (!rc) rc = cilqr_rollout_risk_device(h_, st, B, N, M, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, po, max_risk_,
                                              d + L.base, d + L.risk, (int32_t*)(d + L.hits), d + L.total);
    } else {
      if (!rc) rc = cilqr_rollout_batch_device(h_, st, B, N, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, d + L.Xr, d + L.Ur);
      if (!rc) rc = cilqr_score_rollouts_device(h_, st, B, N, M, S, d + L.Xr, d + L.Ur, d + L.poly, d + L.fl, po, max_risk_, d + L.rows, d + L.risk, d + L.total);
    }
  }
  size_t total_at = plain && !scored ? L.J : L.total;  // each check on top takes the total before it as its base, NaN staying NaN
  if (cmap_checked && !rc) {  // the covariance against the map: Sigma_t of the chance call placed on the nodes
    rc = cilqr_chance_risk_map_device(h_, st, B, N, (int)cmap_weights_.size(), d + L.X, d + L.csig, d + L.qn, d + L.qw, cmap_threshold_,
                                      (cmap_sum_ ? CILQR_CHANCE_MAP_BOUND_SUM : 0u) | (cmap_unknown_hits_ ? CILQR_CHANCE_MAP_UNKNOWN_HITS : 0u),
                                      cmap_max_risk_, d + total_at, d + L.cmrisk, d + L.cmstep, nullptr, nullptr, d + L.cmtotal);
    total_at = L.cmtotal;
  }
  const bool map_checked = map_check_ && map_set_ && (noise_fused_ || cov_check_);
  if (map_checked && !rc) {  // the map's say on top of the obstacles': base = their total
    rc = cilqr_rollout_risk_map_device(h_, st, B, N, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, map_threshold_,
                                       map_unknown_hits_ ? CILQR_MAP_RISK_UNKNOWN_HITS : 0u, map_max_risk_, d + total_at, d + L.mrisk,
                                       (int32_t*)(d + L.mhits), (int32_t*)(d + L.munk), d + L.mtotal);
    total_at = L.mtotal;
  }
  if (!rc) rc = cilqr_argmin_device(h_, st, B, d + total_at, d + L.pair);
  if (rc) {
    const std::string msg = cilqr_last_error();
    (void)hipStreamSynchronize(st);
    throw std::runtime_error((plain ? "run_candidates (chance tightening): " : "run_candidates (pose-noise check): ") + msg);
  }
  double pair[2] = {0.0, -1.0};
  last_scores.clear();
  last_step_hits.clear();
  last_risk.clear();
  last_chance_risk.clear();
  last_step_risk.clear();
  down(pair, L.pair, sizeof(pair));
  if (cov_check_) {
    last_chance_risk.assign((size_t)B * CILQR_CHANCE_FIELDS, 0.0);
    last_step_risk.assign((size_t)B * N, 0.0);
    down(last_chance_risk.data(), L.crisk, last_chance_risk.size() * sizeof(double));
    down(last_step_risk.data(), L.cstep, last_step_risk.size() * sizeof(double));
  } else if (!plain) {
    last_risk.assign((size_t)B * risk_fields, 0.0);
    down(last_risk.data(), L.risk, last_risk.size() * sizeof(double));
  }
  std::vector<double> tg_rows;
  last_tighten.clear();
  last_tighten_risk_before.clear();
  last_tighten_map.clear();
  last_tighten_map_risk_before.clear();
  last_track_map.clear();
  if (tightened) fetch_tighten(st, d, B, tg_rows);
  if (scored) {
    last_scores.assign((size_t)B * CILQR_SCORE_FIELDS, 0.0);
    down(last_scores.data(), L.score, last_scores.size() * sizeof(double));
  }
  if (noise_fused_ && !cov_check_) {
    last_step_hits.assign((size_t)B * N, 0);
    down(last_step_hits.data(), L.hits, last_step_hits.size() * sizeof(int32_t));
  }
  last_chance_map_risk.clear();
  last_map_step_risk.clear();
  if (cmap_checked) {
    last_chance_map_risk.assign((size_t)B * CILQR_CHANCE_MAP_FIELDS, 0.0);
    last_map_step_risk.assign((size_t)B * N, 0.0);
    down(last_chance_map_risk.data(), L.cmrisk, last_chance_map_risk.size() * sizeof(double));
    down(last_map_step_risk.data(), L.cmstep, last_map_step_risk.size() * sizeof(double));
  }
  last_map_risk.clear();
  last_map_step_hits.clear();
  last_map_unknown_hits.clear();
  if (map_checked) {
    last_map_risk.assign((size_t)B * CILQR_MAP_RISK_FIELDS, 0.0);
    last_map_step_hits.assign((size_t)B * N, 0);
    last_map_unknown_hits.assign((size_t)B * N, 0);
    down(last_map_risk.data(), L.mrisk, last_map_risk.size() * sizeof(double));
    down(last_map_step_hits.data(), L.mhits, last_map_step_hits.size() * sizeof(int32_t));
    down(last_map_unknown_hits.data(), L.munk, last_map_unknown_hits.size() * sizeof(int32_t));
  }
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (tightened) keep_tighten_risk(B, tg_rows);
  const int best = (int)pair[1];
  if (best < 0) return -1;  // every candidate rejected: results and warm start stay
  Matrix Xb(4, N + 1);
  int32_t iters = 0, status = 0;
  double J = 0.0;
  down(Xb.a.data(), L.X + (size_t)best * 4 * (N + 1), Xb.a.size() * sizeof(double));
  std::vector<double> Ub((size_t)2 * N);
  down(Ub.data(), L.U + (size_t)best * 2 * N, Ub.size() * sizeof(double));
  down(&J, L.J + (size_t)best, sizeof(double));
  hip_check(hipMemcpyAsync(&iters, (int32_t*)(d + L.iters) + best, sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  hip_check(hipMemcpyAsync(&status, (int32_t*)(d + L.status) + best, sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  X_result = Xb;
  control_seq_.a = Ub;
  U_result = control_seq_;
  ref_traj_result = Matrix(2, n_ref[best]);
  for (int i = 0; i < 2 * n_ref[best]; ++i) ref_traj_result.a[i] = ref[(size_t)best * 2 * W + i];
  last_iterations = iters;
  last_exit = status;
  last_cost = J;
  return best;
}

// run_candidates under set_sample_covariance_check: the analytic chain in the compact sampled form, in a device block of its own
// (grown when a call needs more), on the checks' stream.
int iLQR::run_candidates_sample_covariance(int B, const std::vector<double>& ego_states) {
  const int N = params.horizon;
  if (!n_samples_) throw std::logic_error(kSampleCovarianceWithoutSamples);
  if (!noise_.empty()) throw std::logic_error(kSampleCovarianceWithNoise);
  std::vector<double> U((size_t)B * 2 * N), poly((size_t)B * CILQR_POLY_COEFFS), fl((size_t)B * 2);
  const int W = params.num_of_local_wpts;
  std::vector<double> ref((size_t)B * 2 * W);
  std::vector<int32_t> n_ref(B);
  check(cilqr_local_plan_batch(h_, B, global_plan_.cols, global_plan_.a.data(), 0, ego_states.data(), poly.data(), fl.data(),
                               ref.data(), n_ref.data()), "cilqr_local_plan_batch");
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 2 * N; ++i) U[(size_t)b * 2 * N + i] = control_seq_.a[i];
  std::vector<double> nom_pose, nom_dim, samp_off;  // (alive until the stream has been waited for)
  const int n_obs = pack_sampled(B, nom_pose, nom_dim, samp_off), ns = n_samples_;
  const bool cmap_checked = cmap_check_ && map_set_;
  const size_t Q = cmap_checked ? cmap_weights_.size() : 0;
  struct { size_t x0, U, poly, fl, pose, dim, soff, X, J, iters, status, k, K, ok, score, base, s0, W, crisk, ctotal, csig, srisk, stotal, qn, qw, cmrisk, cmtotal, pair, end; } L;
  size_t o = 0;
  const auto take = [&o](size_t doubles) { const size_t at = o; o += (doubles + 1) & ~(size_t)1; return at; };
  L.x0 = take((size_t)B * 4); L.U = take(U.size()); L.poly = take(poly.size()); L.fl = take(fl.size());
  L.pose = take(nom_pose.size()); L.dim = take(nom_dim.size()); L.soff = take(samp_off.size());
  L.X = take((size_t)B * 4 * (N + 1)); L.J = take(B); L.iters = take(B); L.status = take(B);
  L.k = take((size_t)B * 2 * N); L.K = take((size_t)B * 8 * N); L.ok = take(B);
  L.score = take((size_t)B * CILQR_SCORE_FIELDS); L.base = take(B);
  L.s0 = take(16); L.W = take(16); L.crisk = take((size_t)B * CILQR_CHANCE_FIELDS); L.ctotal = take(B);
  L.csig = take((size_t)B * (N + 1) * 16); L.srisk = take((size_t)B * CILQR_CRS_FIELDS); L.stotal = take(B);
  L.qn = take(Q * 3); L.qw = take(Q); L.cmrisk = take(cmap_checked ? (size_t)B * CILQR_CHANCE_MAP_FIELDS : 0); L.cmtotal = take(cmap_checked ? B : 0);
  L.pair = take(2);
  L.end = o;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  if (!noise_stream_) {
    hipStream_t created;
    hip_check(hipStreamCreateWithFlags(&created, hipStreamNonBlocking), "hipStreamCreateWithFlags");
    noise_stream_ = created;
  }
  hipStream_t st = (hipStream_t)noise_stream_;
  if (L.end > scov_cap_) {
    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (scov_dev_) hip_check(hipFree(scov_dev_), "hipFree");
    scov_dev_ = nullptr; scov_cap_ = 0;
    hip_check(hipMalloc(&scov_dev_, L.end * sizeof(double)), "hipMalloc");
    scov_cap_ = L.end;
  }
  double* d = (double*)scov_dev_;
  const auto up = [&](size_t at, const void* src, size_t doubles) {
    if (doubles) hip_check(hipMemcpyAsync(d + at, src, doubles * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  };
  const auto down = [&](void* dst, size_t at, size_t bytes) {
    hip_check(hipMemcpyAsync(dst, d + at, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  };
  up(L.x0, ego_states.data(), (size_t)B * 4);
  up(L.U, U.data(), U.size());
  up(L.poly, poly.data(), poly.size());
  up(L.fl, fl.data(), fl.size());
  up(L.pose, nom_pose.data(), nom_pose.size());
  up(L.dim, nom_dim.data(), nom_dim.size());
  up(L.soff, samp_off.data(), samp_off.size());
  up(L.s0, scov_sigma0_, 16);
  if (scov_has_W_) up(L.W, scov_W_, 16);
  if (cmap_checked) { up(L.qn, cmap_nodes_.data(), cmap_nodes_.size()); up(L.qw, cmap_weights_.data(), cmap_weights_.size()); }
  const double w = sample_weight();
  int rc = cilqr_solve_batch_sampled_device(h_, st, B, N, n_obs, ns, d + L.x0, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim, d + L.soff, w,
                                            d + L.X, d + L.J, (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
  if (!rc) rc = cilqr_gains_batch_sampled_device(h_, st, B, N, n_obs, ns, d + L.X, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                 d + L.soff, w, scov_lamb_, d + L.k, d + L.K, (int32_t*)(d + L.ok));
  if (!rc) rc = cilqr_score_batch_sampled_device(h_, st, B, N, n_obs, ns, d + L.X, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                 d + L.soff, w, 1.0, d + L.score, d + L.base);
  // the chain alone (M = 0): every Sigma_t, and the steps whose U_t or K_t is not finite marked in its total
  if (!rc) rc = cilqr_chance_risk_device(h_, st, B, N, 0, d + L.X, d + L.U, d + L.K, d + L.s0, 0, scov_has_W_ ? d + L.W : nullptr, nullptr,
                                         scov_sum_ ? CILQR_CHANCE_BOUND_SUM : 0u, scov_max_risk_, d + L.base, d + L.crisk, nullptr, nullptr,
                                         d + L.csig, d + L.ctotal);
  if (!rc) rc = cilqr_chance_risk_sampled_device(h_, st, B, N, n_obs, ns, d + L.X, d + L.csig, d + L.pose, d + L.dim, d + L.soff,
                                                 scov_sum_ ? CILQR_CHANCE_SAMPLED_BOUND_SUM : 0u, scov_max_risk_, d + L.ctotal, d + L.srisk,
                                                 nullptr, nullptr, nullptr, d + L.stotal);
  size_t total_at = L.stotal;
  if (cmap_checked && !rc) {
    rc = cilqr_chance_risk_map_device(h_, st, B, N, (int)Q, d + L.X, d + L.csig, d + L.qn, d + L.qw, cmap_threshold_,
                                      (cmap_sum_ ? CILQR_CHANCE_MAP_BOUND_SUM : 0u) | (cmap_unknown_hits_ ? CILQR_CHANCE_MAP_UNKNOWN_HITS : 0u),
                                      cmap_max_risk_, d + total_at, d + L.cmrisk, nullptr, nullptr, nullptr, d + L.cmtotal);
    total_at = L.cmtotal;
  }
  if (!rc) rc = cilqr_argmin_device(h_, st, B, d + total_at, d + L.pair);
  if (rc) {
    const std::string msg = cilqr_last_error();
    (void)hipStreamSynchronize(st);
    throw std::runtime_error("run_candidates (sample covariance check): " + msg);
  }
  double pair[2] = {0.0, -1.0};
  down(pair, L.pair, sizeof(pair));
  last_scores.assign((size_t)B * CILQR_SCORE_FIELDS, 0.0);
  down(last_scores.data(), L.score, last_scores.size() * sizeof(double));
  last_chance_risk_sampled.assign((size_t)B * CILQR_CRS_FIELDS, 0.0);
  down(last_chance_risk_sampled.data(), L.srisk, last_chance_risk_sampled.size() * sizeof(double));
  last_chance_map_risk.clear();
  if (cmap_checked) {
    last_chance_map_risk.assign((size_t)B * CILQR_CHANCE_MAP_FIELDS, 0.0);
    down(last_chance_map_risk.data(), L.cmrisk, last_chance_map_risk.size() * sizeof(double));
  }
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  const int best = (int)pair[1];
  if (best < 0) return -1;  // every candidate rejected: results and warm start stay
  Matrix Xb(4, N + 1);
  std::vector<double> Ub((size_t)2 * N);
  int32_t iters = 0, status = 0;
  double J = 0.0;
  down(Xb.a.data(), L.X + (size_t)best * 4 * (N + 1), Xb.a.size() * sizeof(double));
  down(Ub.data(), L.U + (size_t)best * 2 * N, Ub.size() * sizeof(double));
  down(&J, L.J + (size_t)best, sizeof(double));
  hip_check(hipMemcpyAsync(&iters, (int32_t*)(d + L.iters) + best, sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  hip_check(hipMemcpyAsync(&status, (int32_t*)(d + L.status) + best, sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  X_result = Xb;
  control_seq_.a = Ub;
  U_result = control_seq_;
  ref_traj_result = Matrix(2, n_ref[best]);
  for (int i = 0; i < 2 * n_ref[best]; ++i) ref_traj_result.a[i] = ref[(size_t)best * 2 * W + i];
  last_iterations = iters;
  last_exit = status;
  last_cost = J;
  return best;
}

// The rounds behind a solve whose arrays lie in the device block: gains and covariance chain of the current plan against the ORIGINAL
// obstacles `po`, the inflated dense table, the re-solve on it from the U the solve before left.  Sigma0, W and obs_cov travel here.
int iLQR::tighten_rounds(void* stream, double* d, int B, const cilqr_obstacles* po) {
  const int N = params.horizon, M = (int)obstacles_.size();
  hipStream_t st = (hipStream_t)stream;
  const NoiseLayout& L = nl_;
  const auto up = [&](size_t at, const void* src, size_t doubles) {
    hip_check(hipMemcpyAsync(d + at, src, doubles * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  };
  if (tighten_ || map_tighten_) up(L.ts0, tg_sigma0_, 16);
  if ((tighten_ || map_tighten_) && tg_has_W_) up(L.tW, tg_W_, 16);
  if (tighten_ && !obs_cov_packed_.empty()) up(L.tcov, obs_cov_packed_.data(), obs_cov_packed_.size());
  cilqr_obstacles inflated{};
  inflated.pose = d + L.tpose;
  inflated.dim = d + L.tdim;
  inflated.batch_stride = (int64_t)M * N;
  inflated.obstacle_stride = N;
  inflated.step_stride = 1;
  // with both tightenings on one round serves both and re-solves once (the setters made the two round counts agree); so it is with the
  // track map beside them: rasterise along the plan, tighten the RASTERISED layers, one re-solve
  const bool trk_on = track_map_on();
  const int Ms = trk_on && !tm_ellipses_ ? 0 : M;  // what the solves read
  const cilqr_obstacles* pos = Ms ? po : nullptr;
  const bool obs_on = tighten_ && M > 0, map_on = map_tightened(), chain = obs_on || map_on;
  const int rounds = obs_on ? tg_rounds_ : map_on ? mt_rounds_ : tm_rounds_;
  const bool layers_on = map_on || trk_on;
  const size_t cells = layers_on ? (size_t)unc_.geom.rows * unc_.geom.cols : 0;
  // map_dev_: the original layer, one layer per candidate, and with both kinds of round a second one per candidate
  float* first_layers = map_dev_ + cells;
  float* second_layers = first_layers + (size_t)max_candidates_ * cells;
  const cilqr_uncertainty_map original = layers_on ? device_map(false) : cilqr_uncertainty_map{};
  const cilqr_uncertainty_map rastered = layers_on ? device_map(true) : cilqr_uncertainty_map{};
  cilqr_uncertainty_map layers = rastered;  // what the re-solve reads
  if (map_on && trk_on) layers.layer = second_layers;
  const bool trk_cov = trk_on && !obs_cov_packed_.empty();
  if (trk_cov) up(L.tkcov, obs_cov_packed_.data(), obs_cov_packed_.size());
  int rc = CILQR_OK;
  for (int r = 0; r < rounds && !rc; ++r) {
    if (chain) {
      rc = cilqr_gains_batch_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, tg_lamb_, d + L.k, d + L.K, (int32_t*)(d + L.ok));
      if (!rc) rc = cilqr_chance_risk_device(h_, st, B, N, M, d + L.X, d + L.U, d + L.K, d + L.ts0, 0, tg_has_W_ ? d + L.tW : nullptr, po, 0u, 1.0,
                                             nullptr, d + L.trisk, nullptr, nullptr, d + L.tsig, nullptr);
    }
    if (!rc && obs_on)
      rc = cilqr_tighten_obstacles_device(h_, st, B, N, M, d + L.X, d + L.tsig, po, obs_cov_packed_.empty() ? nullptr : d + L.tcov, tg_kappa_,
                                          tg_cap_, d + L.tpose, d + L.tdim, d + L.tg);
    // the ORIGINAL layer is the one on the handle here: neither the rasterisation nor the inflation compounds over rounds
    if (!rc && trk_on)
      rc = cilqr_rasterize_tracks_device(h_, st, B, N, M, d + L.X, po, trk_cov ? d + L.tkcov : nullptr, tm_inflate_, tm_z_max_, tm_window_, 0u,
                                         first_layers, d + L.tkf);
    if (!rc && map_on && trk_on) rc = cilqr_set_uncertainty_map_device(h_, &rastered);  // the tightening reads the rasterised layers
    if (!rc && map_on) rc = cilqr_tighten_map_device(h_, st, B, N, d + L.X, d + L.tsig, mt_kappa_, mt_cap_, trk_on ? second_layers : first_layers, d + L.tmg);
    if (!rc && layers_on) rc = cilqr_set_uncertainty_map_device(h_, &layers);
    if (!rc) rc = cilqr_solve_batch_obstacles_device(h_, st, B, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, obs_on ? &inflated : pos, d + L.X,
                                                     d + L.J, (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
    if (layers_on) {  // the original map is back on the handle whatever happened: what follows judges the plan against it
      const int back = cilqr_set_uncertainty_map_device(h_, &original);  // (a success leaves cilqr_last_error as it is)
      if (!rc) rc = back;
    }
  }
  return rc;
}

void iLQR::fetch_tighten(void* stream, double* d, int B, std::vector<double>& risk_rows) {
  risk_rows.assign((size_t)B * CILQR_CHANCE_FIELDS, 0.0);
  if (map_tightened()) {
    last_tighten_map.assign((size_t)B * CILQR_TIGHTEN_MAP_FIELDS, 0.0);
    hip_check(hipMemcpyAsync(last_tighten_map.data(), d + nl_.tmg, last_tighten_map.size() * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync");
  }
  if (tighten_ && !obstacles_.empty()) {
    last_tighten.assign((size_t)B * CILQR_TIGHTEN_FIELDS, 0.0);
    hip_check(hipMemcpyAsync(last_tighten.data(), d + nl_.tg, last_tighten.size() * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync");
  }
  if (track_map_on()) {
    last_track_map.assign((size_t)B * CILQR_TRACK_MAP_FIELDS, 0.0);
    hip_check(hipMemcpyAsync(last_track_map.data(), d + nl_.tkf, last_track_map.size() * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync");
  }
  if (tighten_ || map_tighten_)  // (the chain ran: the risk row of the plan the last round started from)
    hip_check(hipMemcpyAsync(risk_rows.data(), d + nl_.trisk, risk_rows.size() * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync");
}

void iLQR::keep_tighten_risk(int B, const std::vector<double>& risk_rows) {
  std::vector<double> before(B);
  for (int b = 0; b < B; ++b) before[b] = risk_rows[(size_t)b * CILQR_CHANCE_FIELDS + CILQR_CR_STEP_RISK];
  if (tighten_ && !obstacles_.empty()) last_tighten_risk_before = before;
  if (map_tightened()) last_tighten_map_risk_before = before;
}

// get_optimal_control_seq under set_chance_tightening: the B = 1 solve and its rounds in the device block, one wait.
void iLQR::solve_tightened(const double x_0[4], Matrix& U, const double poly_coeffs[6], const double fl[2]) {
  const int N = params.horizon, M = (int)obstacles_.size();
  check_track_map_conflicts();
  if (n_samples_ && (tighten_ || map_tighten_)) throw std::logic_error(tighten_ ? kTighteningWithSamples : kMapTighteningWithSamples);
  if (noise_horizon_ != N) reserve_noise_buffers();
  const cilqr_obstacles host_obs = obstacle_strides();
  if (tighten_ && M && !obs_cov_.empty() && obs_cov_packed_.empty()) throw std::runtime_error(kObstacleCovarianceSize);
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hipStream_t st = (hipStream_t)noise_stream_;
  double* d = (double*)noise_dev_;
  const NoiseLayout& L = nl_;
  const auto up = [&](size_t at, const void* src, size_t doubles) {
    if (doubles) hip_check(hipMemcpyAsync(d + at, src, doubles * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  };
  const auto down = [&](void* dst, size_t at, size_t bytes) {
    hip_check(hipMemcpyAsync(dst, d + at, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  };
  up(L.x0, x_0, 4);
  up(L.U, U.a.data(), U.a.size());
  up(L.poly, poly_coeffs, CILQR_POLY_COEFFS);
  up(L.fl, fl, 2);
  up(L.pose, obs_pose_.data(), obs_pose_.size());
  up(L.dim, obs_dim_.data(), obs_dim_.size());
  cilqr_obstacles obs = host_obs;  // the same strides over the device copies
  obs.pose = d + L.pose;
  obs.dim = d + L.dim;
  const cilqr_obstacles* po = M ? &obs : nullptr;
  const int Ms = track_map_on() && !tm_ellipses_ ? 0 : M;  // (ellipses off: the tracks reach the solve through the map only)
  int rc = cilqr_solve_batch_obstacles_device(h_, st, 1, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, Ms ? po : nullptr, d + L.X, d + L.J,
                                              (int32_t*)(d + L.iters), (int32_t*)(d + L.status), CILQR_FLAG_NONE);
  const bool tightened = (tighten_ && M > 0) || map_tightened() || track_map_on();
  if (!rc && tightened) rc = tighten_rounds(st, d, 1, po);
  if (rc) {
    const std::string msg = cilqr_last_error();
    (void)hipStreamSynchronize(st);
    throw std::runtime_error("run_step (chance tightening): " + msg);
  }
  Matrix Xb(4, N + 1);
  int32_t iters = 0, status = 0;
  double J = 0.0;
  std::vector<double> tg_rows;
  last_tighten.clear();
  last_tighten_risk_before.clear();
  last_tighten_map.clear();
  last_tighten_map_risk_before.clear();
  last_track_map.clear();
  down(Xb.a.data(), L.X, Xb.a.size() * sizeof(double));
  down(U.a.data(), L.U, U.a.size() * sizeof(double));
  down(&J, L.J, sizeof(double));
  down(&iters, L.iters, sizeof(int32_t));
  down(&status, L.status, sizeof(int32_t));
  if (tightened) fetch_tighten(st, d, 1, tg_rows);
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (tightened) keep_tighten_risk(1, tg_rows);
  X_result = Xb;
  last_iterations = iters;
  last_exit = status;
  last_cost = J;
  U_result = U;  // I/iLQR.cpp:244
}

}  // namespace cilqr_host
