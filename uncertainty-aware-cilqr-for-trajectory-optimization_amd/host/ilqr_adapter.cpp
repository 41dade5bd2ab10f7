// ilqr_adapter.cpp — see ilqr_adapter.h.  Host C++ over the C-ABI; the HIP runtime is used for one thing only: the device block
// and the stream of the checks (candidate_layout.h), whose pipeline stays on the device between the C-ABI's _device calls.
#include "ilqr_adapter.h"

#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <stdexcept>
#include <string>

namespace cilqr_host {

namespace {
void check(int rc, const char* what) {
  if (rc != CILQR_OK) throw std::runtime_error(std::string(what) + ": " + cilqr_last_error());
}
void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
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
const char* const kStopFallbackWithoutFootprint =
    "set_stop_fallback needs set_footprint_check: a stop row that no exact check judged is no fallback";
const char* const kFootprintWithSamples =
    "set_footprint_check has no form for sampled obstacles (set_obstacle_samples): it judges rectangles, and a sample has none";
const char* const kSampleCovarianceWithNoise =
    "set_sample_covariance_check and set_pose_noise_check(_fused) are both set: the pose noise is given either as a covariance or as draws";
const char* const kSampleCovarianceWithoutSamples =
    "set_sample_covariance_check has effect with obstacle samples (set_obstacle_samples) only: without samples use set_pose_covariance_check";
}  // namespace

// The checks' device block and the stream everything on it goes to.  `d + at` is the array at offset `at` (in doubles).
struct iLQR::Block {
  double* d;
  hipStream_t st;
  double* operator+(size_t at) const { return d + at; }
  int32_t* i32(size_t at) const { return (int32_t*)(d + at); }
  void up(size_t at, const void* src, size_t doubles) const {
    if (doubles) hip_check(hipMemcpyAsync(d + at, src, doubles * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  }
  void down(void* dst, size_t at, size_t bytes) const {
    hip_check(hipMemcpyAsync(dst, d + at, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  void down_i32(int32_t* dst, size_t at, size_t index) const {
    hip_check(hipMemcpyAsync(dst, i32(at) + index, sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  template <class T>
  void fetch(std::vector<T>& v, size_t at, size_t n) const {  // a last_* vector: sized, then filled from the block
    v.assign(n, T(0));
    down(v.data(), at, n * sizeof(T));
  }
  void wait() const { hip_check(hipStreamSynchronize(st), "hipStreamSynchronize"); }
};

struct iLQR::Candidates {
  std::vector<double> U, poly, fl, ref;
  std::vector<int32_t> n_ref;
};

struct iLQR::Solved {
  Matrix X;
  std::vector<double> U;
  double J = 0.0;
  int32_t iters = 0, status = 0;
};

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
  if (block_stream_) (void)hipStreamSynchronize((hipStream_t)block_stream_);
  if (block_dev_) (void)hipFree(block_dev_);
  if (map_dev_) (void)hipFree(map_dev_);
  if (frame_dev_) (void)hipFree(frame_dev_);
  if (mo_dev_) (void)hipFree(mo_dev_);
  if (trk_dev_) (void)hipFree(trk_dev_);
  if (block_stream_) (void)hipStreamDestroy((hipStream_t)block_stream_);
  cilqr_destroy(h_);
}

void iLQR::set_Obstacle(const std::vector<Obstacle>& obstacles) {
  if (trk_on_) throw std::logic_error("set_map_tracker: the tracker is the one producer of obstacles while it is on: not with set_Obstacle");
  if ((int)obstacles.size() > max_obstacles_) throw std::runtime_error("set_Obstacle: more obstacles than max_obstacles");
  for (const Obstacle& o : obstacles)
    if (o.dimension.rows != 2 || o.relative_pos_array.rows != 4 || o.dimension.cols < params.horizon ||
        o.relative_pos_array.cols < params.horizon)
      throw std::runtime_error("set_Obstacle: dimension must be 2×horizon and relative_pos_array 4×horizon");
  if (tracked_horizon_ >= 0) obs_cov_.clear();  // (the covariance the prediction installed goes with its obstacles)
  tracked_horizon_ = -1;
  obstacles_ = obstacles;
  map_rows_ = 0;
  append_map_rows();  // (the rows of set_map_obstacles stay behind the new set; packs)
}

void iLQR::clear_Obstacle() {
  trk_reset_ = true;  // (the tracker starts over with the next map)
  trk_owns_tracks_ = false;
  last_tracks.clear();
  if (tracked_horizon_ >= 0) obs_cov_.clear();
  tracked_horizon_ = -1;
  tracks_.clear(); track_dims_.clear(); track_cov_.clear(); track_Q_.clear();
  obstacles_.clear();
  map_rows_ = 0;
  append_map_rows();
}

void iLQR::set_tracked_obstacles(const std::vector<double>& tracks, const std::vector<double>& dims, const std::vector<double>& cov,
                                 const std::vector<double>& Q) {
  if (trk_on_) throw std::logic_error("set_map_tracker: one producer of tracks: not with set_tracked_obstacles");
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
  map_rows_ = 0;  // (a run under set_map_obstacles throws while tracks are set: its rows are not kept behind them)
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
  if (was != on) reserve_block_if_used();
}

void iLQR::set_uncertainty_map(const Uncertainty& u) {
  if (u.layer.size() != (size_t)u.geom.rows * u.geom.cols) throw std::runtime_error("set_uncertainty_map: layer size does not match its geometry");
  apply_map(u);
  unc_ = u;  // (kept: set_map_tightening moves the layer between the handle's device copy and this object's)
  map_set_ = true;
  if (mv_on_) given_layer_ = u.layer;
  if (mo_on_) {
    extract_map_obstacles();
    if (trk_on_) track_map_obstacles();
    else append_map_rows();
    if (mv_on_) clear_tracked_movers();
  }
}

void iLQR::set_map_obstacles(double occ_threshold, double gap, int min_cells, double max_size, double pad, int K, bool on) {
  if (on && (occ_threshold != occ_threshold || !(gap >= 0.0 && gap <= 1.7e308) || min_cells < 1 || !(max_size > 0.0) ||
             !(pad >= 0.0 && pad <= 1.7e308) || K < 1 || K > CILQR_MAX_POLYGONS))
    throw std::runtime_error("set_map_obstacles: needs a threshold that is not NaN, gap and pad >= 0 and finite, min_cells >= 1, max_size > 0 and K in 1 ... CILQR_MAX_POLYGONS");
  if (trk_on_ && !on) throw std::logic_error("set_map_tracker: needs set_map_obstacles: switch the tracker off first");
  if (trk_on_ && K > CILQR_TRACK_MAX_DETECTIONS) throw std::runtime_error("set_map_obstacles: K above CILQR_TRACK_MAX_DETECTIONS under set_map_tracker");
  mo_on_ = on;
  if (on) { mo_threshold_ = occ_threshold; mo_gap_ = gap; mo_min_cells_ = min_cells; mo_max_size_ = max_size; mo_pad_ = pad; mo_K_ = K; }
  if (on && map_set_) extract_map_obstacles();
  if (!on) { last_map_obstacles.clear(); memset(last_map_obstacle_counts, 0, sizeof(last_map_obstacle_counts)); }
  if (trk_on_) return;  // (the rows reach the tracker with the next map; no static row is appended)
  if (on ? map_set_ : map_rows_ > 0) append_map_rows();
}

void iLQR::set_map_tracker(const cilqr_track_filter& f, int slots, bool on) {
  if (!on && trk_on_ && mv_on_) throw std::logic_error("set_mover_clearing: needs set_map_tracker: switch the clearing off first");
  if (!on) {
    if (trk_on_) {
      trk_on_ = false;
      drop_tracker_tracks();
      if (mo_on_ && map_set_) append_map_rows();  // the static rows again
    }
    return;
  }
  if (!mo_on_) throw std::logic_error("set_map_tracker: needs set_map_obstacles");
  if (mo_K_ > CILQR_TRACK_MAX_DETECTIONS) throw std::runtime_error("set_map_tracker: the K of set_map_obstacles is above CILQR_TRACK_MAX_DETECTIONS");
  if (slots < 1 || slots > CILQR_TRACK_MAX_SLOTS || slots > max_obstacles_)
    throw std::runtime_error("set_map_tracker: slots outside 1 ... min(CILQR_TRACK_MAX_SLOTS, max_obstacles)");
  if (!trk_on_ && (tracked_horizon_ >= 0 || !obs_cov_.empty()))
    throw std::logic_error("set_map_tracker: one producer of tracks: not with set_tracked_obstacles or set_obstacle_covariance in force");
  if (!trk_on_ && (int)obstacles_.size() > map_rows_)
    throw std::logic_error("set_map_tracker: the tracker is the one producer of obstacles: call clear_Obstacle first");
  if (!(f.dt > 0.0 && f.dt <= 1.7e308) || !(f.gate2 >= 0.0) || !(f.v_min >= 0.0) || !(f.theta_var_slow >= 0.0) || f.min_hits < 1 || f.max_misses < 0)
    throw std::runtime_error("set_map_tracker: a filter cilqr_track_update rejects (dt > 0, gate2, v_min, theta_var_slow >= 0, min_hits >= 1, max_misses >= 0)");
  if (hipSetDevice(device_) != hipSuccess) throw std::runtime_error("set_map_tracker: hipSetDevice failed");
  if (!trk_on_ || slots != trk_slots_) {
    if (trk_dev_) (void)hipFree(trk_dev_);
    trk_dev_ = nullptr;
    const size_t need = ((size_t)slots * (CILQR_TRACK_STATE + 24) + CILQR_TRACK_WORLD_FIELDS) * sizeof(double) + CILQR_TRACK_MAX_DETECTIONS * sizeof(int32_t);
    if (hipMalloc(&trk_dev_, need) != hipSuccess) throw std::runtime_error("set_map_tracker: hipMalloc failed");
    trk_reset_ = true;
  }
  const bool was = trk_on_;
  if (!was) {  // the static rows leave: the tracker's rows stand in their place
    trk_reset_ = true;
    obstacles_.erase(obstacles_.end() - map_rows_, obstacles_.end());
    map_rows_ = 0;
    pack_obstacles();
  }
  trk_f_ = f;
  trk_slots_ = slots;
  trk_on_ = true;
  if (!was && map_set_) { extract_map_obstacles(); track_map_obstacles(); }  // (the map already set is the first tick)
}

void iLQR::drop_tracker_tracks() {
  if (trk_owns_tracks_) {
    if (tracked_horizon_ >= 0) obs_cov_.clear();
    tracked_horizon_ = -1;
    tracks_.clear(); track_dims_.clear(); track_cov_.clear(); track_Q_.clear();
    obstacles_.clear();
    map_rows_ = 0;
    pack_obstacles();
  }
  trk_owns_tracks_ = false;
  last_tracks.clear();
  memset(last_track_counts, 0, sizeof(last_track_counts));
}

// One tick on the boxes extract_map_obstacles left on the device (null stream, behind them), then the table's output rows come back and
// the confirmed ones are installed as set_tracked_obstacles would install them.
void iLQR::track_map_obstacles() {
  const size_t M = (size_t)trk_slots_;
  double *state = (double*)trk_dev_, *world = state + M * CILQR_TRACK_STATE, *track = world + CILQR_TRACK_WORLD_FIELDS, *dim = track + M * 6,
         *cov = dim + M * 2;
  int32_t* assign = (int32_t*)(cov + M * 16);
  check(cilqr_track_update_device(h_, nullptr, 1, trk_slots_, mo_K_, mo_boxes_dev_, mo_n_out_dev_ + 2, 4, &trk_f_, state, state, world,
                                  trk_reset_ ? CILQR_TRACK_RESET : 0u, assign, track, dim, cov),
        "cilqr_track_update_device");
  trk_reset_ = false;
  std::vector<double> host(M * (CILQR_TRACK_STATE + 24) + CILQR_TRACK_WORLD_FIELDS);
  if (hipMemcpy(host.data(), trk_dev_, host.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error("set_map_tracker: HIP runtime call failed");
  const double *hs = host.data(), *hw = hs + M * CILQR_TRACK_STATE, *ht = hw + CILQR_TRACK_WORLD_FIELDS, *hd = ht + M * 6, *hc = hd + M * 2;
  memcpy(last_track_counts, hw, sizeof(last_track_counts));
  last_tracks.clear();
  std::vector<double> tracks, dims, covs;
  for (size_t m = 0; m < M; ++m) {
    const double* row = hs + m * CILQR_TRACK_STATE;
    if (!(row[CILQR_TS_ID] >= 0.0 && row[CILQR_TS_HITS] >= (double)trk_f_.min_hits)) continue;  // filler
    tracks.insert(tracks.end(), ht + 6 * m, ht + 6 * m + 6);
    dims.insert(dims.end(), hd + 2 * m, hd + 2 * m + 2);
    covs.insert(covs.end(), hc + 16 * m, hc + 16 * m + 16);
    const double r[8] = {row[CILQR_TS_ID], ht[6 * m], ht[6 * m + 1], ht[6 * m + 2], ht[6 * m + 3], hd[2 * m], hd[2 * m + 1], (double)m};
    last_tracks.insert(last_tracks.end(), r, r + 8);
  }
  if (tracks.empty()) {  // nothing confirmed: no obstacle at all
    if (trk_owns_tracks_) {
      if (tracked_horizon_ >= 0) obs_cov_.clear();
      tracked_horizon_ = -1;
      tracks_.clear(); track_dims_.clear(); track_cov_.clear(); track_Q_.clear();
      obstacles_.clear();
      pack_obstacles();
    }
    trk_owns_tracks_ = false;
    return;
  }
  tracks_ = tracks; track_dims_ = dims; track_cov_ = covs; track_Q_.clear();
  install_tracked();
  trk_owns_tracks_ = true;
}

// The device forms on a block of this object's own (the layer, d2, work, label_out, then n_out, comp, boxes and the pose), grown when a
// larger map or K comes: a map's three arrays of 4 bytes a cell do not fit the arena of a handle made for a few candidates, which is
// sized by solves.  The results are those of the host forms, bit for bit.
void iLQR::extract_map_obstacles() {
  const cilqr_map_geom& g = unc_.geom;
  const size_t cells = (size_t)g.rows * g.cols, ints = (4 * cells + 4 + 1) / 2 * 2, K = (size_t)mo_K_;
  const size_t doubles = K * (CILQR_MAP_OBSTACLE_FIELDS + 5) + 3 + CILQR_CLEAR_MOVERS_FIELDS, need = ints * sizeof(int32_t) + doubles * sizeof(double);
  const char* what = "set_map_obstacles: HIP runtime call failed";
  if (hipSetDevice(device_) != hipSuccess) throw std::runtime_error(what);
  if (need > mo_dev_cap_) {
    if (mo_dev_) (void)hipFree(mo_dev_);
    mo_dev_ = nullptr; mo_dev_cap_ = 0;
    if (hipMalloc(&mo_dev_, need) != hipSuccess) throw std::runtime_error("set_map_obstacles: hipMalloc failed");
    mo_dev_cap_ = need;
  }
  float* layer = (float*)mo_dev_;
  int32_t *d2 = (int32_t*)mo_dev_ + cells, *work = d2 + cells, *label = work + cells, *n_out = label + cells;
  double *comp = (double*)((int32_t*)mo_dev_ + ints), *boxes = comp + K * CILQR_MAP_OBSTACLE_FIELDS, *pose_dev = boxes + K * 5;
  mo_boxes_dev_ = boxes; mo_n_out_dev_ = n_out;  // (where set_map_tracker reads its detections and their count)
  const double r = mo_gap_ / g.res, r2 = floor(r * r);
  const int gap2 = r2 < 2147483646.0 ? (int)r2 : 2147483646;
  const double pose[3] = {unc_.pose_x, unc_.pose_y, unc_.pose_theta};
  // (the null stream: each copy below waits for what was enqueued before it)
  const std::vector<float>& given = mv_on_ && given_layer_.size() == cells ? given_layer_ : unc_.layer;  // (under set_mover_clearing unc_ holds the cleared layer)
  if (hipMemcpy(layer, given.data(), cells * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pose_dev, pose, sizeof(pose), hipMemcpyHostToDevice) != hipSuccess)
    throw std::runtime_error(what);
  check(cilqr_map_distance_device(h_, nullptr, 1, layer, 0, &g, mo_threshold_, 0u, d2, nullptr), "cilqr_map_distance_device");
  check(cilqr_map_obstacles_device(h_, nullptr, 1, d2, &g, gap2, 0u, pose_dev, 0, mo_K_, mo_min_cells_, mo_max_size_, mo_pad_, work, label, n_out,
                                   comp, boxes, nullptr, nullptr),
        "cilqr_map_obstacles_device");
  std::vector<double> rows(K * 5);
  if (hipMemcpy(last_map_obstacle_counts, n_out, 4 * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(rows.data(), boxes, rows.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error(what);
  if (last_map_obstacle_counts[2] < 0) throw std::runtime_error("set_map_obstacles: cilqr_map_obstacles ran out of a loop bound (CILQR_ERR_INTERNAL)");
  last_map_obstacles.assign(rows.begin(), rows.begin() + (size_t)5 * last_map_obstacle_counts[2]);
}

int iLQR::mover_halo2(double res) const {
  const double r = mv_halo_ / res, r2 = floor(r * r);
  if (!(r2 <= (double)CILQR_CLEAR_MOVERS_MAX_HALO2)) throw std::runtime_error("set_mover_clearing: halo beyond CILQR_CLEAR_MOVERS_MAX_HALO2 cells^2 at this map's resolution");
  return (int)r2;
}

void iLQR::set_mover_clearing(double v_clear, double halo, float fill, bool on) {
  if (!on) {
    const bool was = mv_on_;
    mv_on_ = false;
    memset(last_mover_clearing, 0, sizeof(last_mover_clearing));
    if (was && map_set_ && given_layer_.size() == unc_.layer.size()) {  // the layer as given is the map again
      unc_.layer = given_layer_;
      apply_map(unc_);
    }
    given_layer_.clear();
    return;
  }
  if (!trk_on_) throw std::logic_error("set_mover_clearing: needs set_map_tracker");
  if (!(v_clear >= 0.0) || !(halo >= 0.0 && halo <= 1.7e308) || (fill == fill && fill - fill != 0.0f))
    throw std::runtime_error("set_mover_clearing: needs v_clear >= 0, halo >= 0 and finite, and a fill that is finite or NaN");
  const double keep = mv_halo_;
  mv_halo_ = halo;
  if (map_set_) {
    try { (void)mover_halo2(unc_.geom.res); } catch (...) { mv_halo_ = keep; throw; }
  }
  mv_v_clear_ = v_clear; mv_fill_ = fill;
  const bool was = mv_on_;
  mv_on_ = true;
  if (!map_set_) return;
  if (!was) given_layer_ = unc_.layer;
  // (the map already set: its labels, rows and tracks are in the device blocks as the last tick left them; the layer as given goes up again)
  const size_t cells = given_layer_.size();
  if (hipSetDevice(device_) != hipSuccess || hipMemcpy(mo_dev_, given_layer_.data(), cells * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    throw std::runtime_error("set_mover_clearing: HIP runtime call failed");
  clear_tracked_movers();
}

// Behind the tick (null stream): the layer as given is still at the head of mo_dev_, the labels and comp lie behind it, assign and the
// table in trk_dev_.  In place on that copy; the cleared layer and the fields come back, and the cleared layer becomes the map.
void iLQR::clear_tracked_movers() {
  const cilqr_map_geom& g = unc_.geom;
  const size_t cells = (size_t)g.rows * g.cols, ints = (4 * cells + 4 + 1) / 2 * 2, K = (size_t)mo_K_, M = (size_t)trk_slots_;
  const int halo2 = mover_halo2(g.res);
  float* layer = (float*)mo_dev_;
  const int32_t* label = (const int32_t*)mo_dev_ + 3 * cells;
  const double* comp = (const double*)((int32_t*)mo_dev_ + ints);
  double* fields = (double*)comp + K * (CILQR_MAP_OBSTACLE_FIELDS + 5) + 3;
  const double* state = (const double*)trk_dev_;
  const int32_t* assign = (const int32_t*)(state + M * (CILQR_TRACK_STATE + 24) + CILQR_TRACK_WORLD_FIELDS);
  check(cilqr_clear_movers_device(h_, nullptr, 1, layer, 0, &g, label, mo_K_, comp, trk_slots_, assign, state, trk_f_.min_hits, mv_v_clear_, nullptr,
                                  halo2, mv_fill_, layer, nullptr, fields),
        "cilqr_clear_movers_device");
  unc_.layer.resize(cells);
  if (hipMemcpy(unc_.layer.data(), layer, cells * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(last_mover_clearing, fields, sizeof(last_mover_clearing), hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error("set_mover_clearing: HIP runtime call failed");
  apply_map(unc_);
}

void iLQR::append_map_rows() {
  obstacles_.erase(obstacles_.end() - map_rows_, obstacles_.end());
  map_rows_ = 0;
  const int N = params.horizon, n = trk_on_ ? 0 : (int)(last_map_obstacles.size() / 5);  // (under set_map_tracker the rows reach the solve as tracks)
  if ((int)obstacles_.size() + n > max_obstacles_) {
    pack_obstacles();
    throw std::runtime_error("set_map_obstacles: the obstacles of set_Obstacle and the rows from the map exceed max_obstacles");
  }
  for (int k = 0; k < n; ++k) {
    const double* b = &last_map_obstacles[(size_t)5 * k];
    Matrix d(2, N), r(4, N);
    for (int t = 0; t < N; ++t) {
      d(0, t) = b[3]; d(1, t) = b[4];
      r(0, t) = b[0]; r(1, t) = b[1]; r(2, t) = 0.0; r(3, t) = b[2];
    }
    obstacles_.emplace_back(params, d, r);
  }
  map_rows_ = n;
  map_rows_horizon_ = N;
  pack_obstacles();
}

void iLQR::check_map_obstacle_conflicts() const {
  if (trk_on_ && n_samples_ > 0) throw std::logic_error("set_map_tracker: the tracks have no samples: not with set_obstacle_samples");
  if (mo_on_ && !trk_on_ && (n_samples_ > 0 || tracked_horizon_ >= 0 || !obs_cov_.empty()))
    throw std::logic_error("set_map_obstacles: the rows from the map have neither samples nor a covariance: not with set_obstacle_samples, "
                           "set_tracked_obstacles or set_obstacle_covariance");
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
  if (block_stream_) (void)hipStreamSynchronize((hipStream_t)block_stream_);  // nothing enqueued may still read the old block
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
  last_map_obstacles.clear();
  memset(last_map_obstacle_counts, 0, sizeof(last_map_obstacle_counts));
  if (trk_on_) { drop_tracker_tracks(); trk_reset_ = true; }  // (the tracks go with their map, and the tracker starts over)
  given_layer_.clear();
  memset(last_mover_clearing, 0, sizeof(last_mover_clearing));
  if (map_rows_ > 0) append_map_rows();  // (the rows go with their map)
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
  refresh_map_rows();
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
  check_map_obstacle_conflicts();
  refresh_map_rows();
  const int N = params.horizon, M = (int)obstacles_.size();
  if (U.rows != 2 || U.cols != N) throw std::runtime_error("get_optimal_control_seq: U must be 2×horizon");
  if (x_local_plan.empty()) throw std::runtime_error("get_optimal_control_seq: empty x_local_plan");
  const double fl[2] = {x_local_plan.front(), x_local_plan.back()};
  if (modes().chain() || modes().track_rounds()) { solve_tightened(x_0, U, poly_coeffs, fl); return; }
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
  if (frame_on_) { run_framed(1, std::vector<double>(ego_state, ego_state + 4), true); return; }
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

CandidateModes iLQR::modes() const {
  CandidateModes m;
  m.noise = !noise_.empty(); m.fused = noise_fused_; m.cov = cov_.on; m.scov = scov_.on; m.sampled = n_samples_ > 0;
  m.cov_judge = obs_cov_check_; m.cmap = cmap_check_; m.map = map_check_;
  m.tighten = tighten_; m.map_tighten = map_tighten_; m.track_map = tm_rounds_ > 0;
  m.min_total = pick_ == CandidatePick::MinTotalCost;
  m.footprint = fp_check_;
  m.map_clearance = mc_check_;
  m.stop_fallback = stop_on_;
  m.map_set = map_set_; m.obstacles = !obstacles_.empty(); m.tracks = tracked_horizon_ >= 0;
  return m;
}

CandidateSizes iLQR::sizes() const {
  CandidateSizes z;
  z.B = max_candidates_; z.N = params.horizon; z.M = max_obstacles_; z.S = noise_.size() / 4;
  z.n_samples = n_samples_; z.n_obs = n_samples_ ? samples_.size() / 3 / n_samples_ : 0;
  z.Q = cmap_weights_.size();
  z.D = stop_decel_.size();
  return z;
}

iLQR::Block iLQR::block() const { return Block{(double*)block_dev_, (hipStream_t)block_stream_}; }

void iLQR::clear_round_fields() {
  last_tighten.clear(); last_tighten_risk_before.clear();
  last_tighten_map.clear(); last_tighten_map_risk_before.clear();
  last_track_map.clear();
}

void iLQR::clear_candidate_fields() {
  clear_round_fields();
  last_scores.clear(); last_risk.clear(); last_step_hits.clear();
  last_map_risk.clear(); last_map_step_hits.clear(); last_map_unknown_hits.clear();
  last_chance_risk.clear(); last_step_risk.clear();
  last_chance_map_risk.clear(); last_map_step_risk.clear();
  last_chance_risk_sampled.clear();
  last_footprint.clear(); last_footprint_clearance.clear();
  last_map_clearance.clear(); last_map_step_clearance.clear();
  last_stop.clear(); last_stop_footprint.clear();
  last_stop_pick = -1; last_stop_level = -1;
}

// The prologue of every run_candidates: LocalPlanner pre-step for all candidates in one device launch (cilqr_local_plan_batch)
// instead of B host fits, and the warm start replicated into [B][2N].
iLQR::Candidates iLQR::plan_candidates(int B, const std::vector<double>& ego_states) {
  const size_t N = params.horizon, W = params.num_of_local_wpts;
  Candidates c;
  c.U.resize((size_t)B * 2 * N); c.poly.resize((size_t)B * CILQR_POLY_COEFFS); c.fl.resize((size_t)B * 2);
  c.ref.resize((size_t)B * 2 * W); c.n_ref.resize(B);
  check(cilqr_local_plan_batch(h_, B, global_plan_.cols, global_plan_.a.data(), 0, ego_states.data(), c.poly.data(), c.fl.data(),
                               c.ref.data(), c.n_ref.data()), "cilqr_local_plan_batch");
  for (int b = 0; b < B; ++b) memcpy(&c.U[(size_t)b * 2 * N], control_seq_.a.data(), 2 * N * sizeof(double));
  return c;
}

// The epilogue of every solve: `U` is where the caller keeps the controls — the warm start, for run_step and run_candidates.
void iLQR::install(const Solved& s, Matrix& U) {
  X_result = s.X;
  U.a = s.U;
  U_result = U;  // I/iLQR.cpp:244
  last_iterations = s.iters;
  last_exit = s.status;
  last_cost = s.J;
}

void iLQR::fetch_solved(const Block& d, int b, Solved& s) const {
  const size_t N = params.horizon;
  s.X = Matrix(4, (int)N + 1);
  s.U.resize(2 * N);
  d.down(s.X.a.data(), layout_.X + (size_t)b * 4 * (N + 1), s.X.a.size() * sizeof(double));
  d.down(s.U.data(), layout_.U + (size_t)b * 2 * N, s.U.size() * sizeof(double));
  d.down(&s.J, layout_.J + (size_t)b, sizeof(double));
  d.down_i32(&s.iters, layout_.iters, b);
  d.down_i32(&s.status, layout_.status, b);
}

int iLQR::run_candidates(const std::vector<double>& ego_states) {
  if (tracked_horizon_ >= 0 && tracked_horizon_ != params.horizon) install_tracked();
  check_map_obstacle_conflicts();
  refresh_map_rows();
  const int B = (int)(ego_states.size() / 4), N = params.horizon, M = (int)obstacles_.size();
  if (B < 1 || B > max_candidates_) throw std::runtime_error("run_candidates: candidate count outside [1, max_candidates]");
  if (global_plan_.cols < 1) throw std::runtime_error("run_candidates: set_global_plan was not called");
  const CandidateModes m = modes();
  if (m.scov && m.track_rounds()) throw std::logic_error(kTrackMapWithSamples);
  if (m.stop_fallback && !m.footprint) throw std::logic_error(kStopFallbackWithoutFootprint);
  if (frame_on_) return run_framed(B, ego_states, false);
  if (m.in_block()) return run_candidates_in_block(B, ego_states, m);
  // the unchecked path: the host-buffer forms on the handle's stream, the pick on the host
  Candidates c = plan_candidates(B, ego_states);
  std::vector<double> X((size_t)B * 4 * (N + 1)), J(B);
  std::vector<int32_t> iters(B), status(B);
  const cilqr_obstacles obs = obstacle_strides();  // one obstacle set for every candidate
  std::vector<double> total, nom_pose, nom_dim, samp_off;
  const int n_obs = n_samples_ ? pack_sampled(B, nom_pose, nom_dim, samp_off) : 0;
  if (n_samples_)
    check(cilqr_solve_batch_sampled(h_, B, N, n_obs, n_samples_, ego_states.data(), c.U.data(), c.poly.data(), c.fl.data(), nom_pose.data(),
                                    nom_dim.data(), samp_off.data(), sample_weight(), X.data(), J.data(), iters.data(), status.data(),
                                    CILQR_FLAG_NONE),
          "cilqr_solve_batch_sampled");
  else
    check(cilqr_solve_batch_obstacles(h_, B, N, M, ego_states.data(), c.U.data(), c.poly.data(), c.fl.data(), M ? &obs : nullptr, X.data(),
                                      J.data(), iters.data(), status.data(), CILQR_FLAG_NONE),
          "cilqr_solve_batch_obstacles");
  clear_candidate_fields();
  if (m.min_total) {  // rank by everything the solve descended along, among the candidates that are safe
    last_scores.resize((size_t)B * CILQR_SCORE_FIELDS);
    total.resize(B);
    if (n_samples_)
      check(cilqr_score_batch_sampled(h_, B, N, n_obs, n_samples_, X.data(), c.U.data(), c.poly.data(), c.fl.data(), nom_pose.data(),
                                      nom_dim.data(), samp_off.data(), sample_weight(), max_collision_, last_scores.data(), total.data()),
            "cilqr_score_batch_sampled");
    else
      check(cilqr_score_batch(h_, B, N, M, X.data(), c.U.data(), c.poly.data(), c.fl.data(), M ? &obs : nullptr, max_collision_,
                              last_scores.data(), total.data()),
            "cilqr_score_batch");
  }
  const std::vector<double>& rank = m.min_total ? total : J;
  int best = 0;  // strict-< first minimum, NaN never wins (the convention of cilqr_argmin_device)
  bool have = false;
  for (int b = 0; b < B; ++b)
    if (rank[b] == rank[b] && (!have || rank[b] < rank[best])) { best = b; have = true; }
  if (m.min_total && !have) return -1;  // every candidate rejected: results and warm start stay
  Solved s;
  s.X = Matrix(4, N + 1);
  memcpy(s.X.a.data(), &X[(size_t)best * 4 * (N + 1)], s.X.a.size() * sizeof(double));
  s.U.assign(&c.U[(size_t)best * 2 * N], &c.U[(size_t)best * 2 * N] + 2 * N);
  s.J = J[best]; s.iters = iters[best]; s.status = status[best];
  install(s, control_seq_);
  ref_traj_result = Matrix(2, c.n_ref[best]);
  memcpy(ref_traj_result.a.data(), &c.ref[(size_t)best * 2 * params.num_of_local_wpts], ref_traj_result.a.size() * sizeof(double));
  return best;
}

// ---- path-aligned planning frame -----------------------------------------------------------------------------------------------------
namespace {
const char kPathFrameInBlock[] =
    "set_path_frame: the stages of the device block (noise, covariance and sampled checks, tightenings, track map, footprint, map "
    "clearance, stop fallback), the tightened run_step and obstacle samples are not framed: switch them or set_path_frame off";
}

void iLQR::set_path_frame(bool on, bool global_inflation) {
  frame_on_ = on;
  frame_global_inflation_ = on && global_inflation;
  last_frames.clear();
  last_frame_info.clear();
}

// run_step and the unchecked path of run_candidates in the frames of their candidates: the host-buffer forms on the handle's stream,
// the pick on the host, as there.  The solve, the score and the map cost are the unframed calls' own; only their inputs differ.
int iLQR::run_framed(int B, const std::vector<double>& ego_states, bool step) {
  const CandidateModes m = modes();
  if (m.in_block() || m.chain() || m.track_rounds() || n_samples_) throw std::logic_error(kPathFrameInBlock);
  if (step) {  // (run_candidates did these before it came here)
    if (tracked_horizon_ >= 0 && tracked_horizon_ != params.horizon) install_tracked();
    check_map_obstacle_conflicts();
    refresh_map_rows();
  }
  const int N = params.horizon, M = (int)obstacles_.size();
  const size_t W = params.num_of_local_wpts, b = B;
  if (control_seq_.rows != 2 || control_seq_.cols != N) throw std::runtime_error("set_path_frame: the warm start must be 2×horizon");
  std::vector<double> frames(b * CILQR_FRAME_DOUBLES), x0(b * 4), poly(b * CILQR_POLY_COEFFS), fl(b * 2), ref(b * 2 * W), U(b * 2 * N);
  std::vector<int32_t> info(B), n_ref(B);
  check(cilqr_local_plan_frames(h_, B, global_plan_.cols, global_plan_.a.data(), 0, ego_states.data(), frames.data(), info.data(), x0.data(),
                                poly.data(), fl.data(), ref.data(), n_ref.data(), nullptr), "cilqr_local_plan_frames");
  for (int c = 0; c < B; ++c) memcpy(&U[(size_t)c * 2 * N], control_seq_.a.data(), 2 * (size_t)N * sizeof(double));
  // the obstacle rows: one set for every candidate in, one dense table per candidate out
  std::vector<double> pose_f(b * M * 4 * N), dim_f(b * M * 2 * N);
  cilqr_obstacles obs_f{pose_f.data(), dim_f.data(), nullptr, (int64_t)M * N, N, 1, 0};
  if (M) {
    const cilqr_obstacles obs = obstacle_strides();
    check(cilqr_frame_obstacles(h_, B, N, M, frames.data(), CILQR_FRAME_DOUBLES, &obs, nullptr,
                                frame_global_inflation_ ? CILQR_FRAME_GLOBAL_INFLATION : 0u, pose_f.data(), dim_f.data(), nullptr),
          "cilqr_frame_obstacles");
  }
  // the map: its pose in every candidate's frame, behind a device copy of the layer; the handle gets its own map back afterwards
  struct RestoreMap {
    iLQR* self; bool armed;
    ~RestoreMap() { if (armed) { try { self->apply_map(self->unc_); } catch (...) {} } }
  } restore{this, false};
  if (map_set_) {
    const double pose[3] = {unc_.pose_x, unc_.pose_y, unc_.pose_theta};
    std::vector<double> poses_f(b * 3);
    check(cilqr_frame_poses(h_, B, 1, frames.data(), CILQR_FRAME_DOUBLES, pose, 0, poses_f.data()), "cilqr_frame_poses");
    const size_t cells = (size_t)unc_.geom.rows * unc_.geom.cols, layer_bytes = (cells * sizeof(float) + 15) / 16 * 16;
    const size_t need = layer_bytes + (size_t)max_candidates_ * 3 * sizeof(double);
    if (hipSetDevice(device_) != hipSuccess) throw std::runtime_error("set_path_frame: hipSetDevice failed");
    if (need > frame_dev_cap_) {
      if (frame_dev_) (void)hipFree(frame_dev_);
      frame_dev_ = nullptr; frame_dev_cap_ = 0;
      if (hipMalloc(&frame_dev_, need) != hipSuccess) throw std::runtime_error("set_path_frame: hipMalloc failed");
      frame_dev_cap_ = need;
    }
    double* poses_dev = (double*)((char*)frame_dev_ + layer_bytes);
    if (hipMemcpy(frame_dev_, unc_.layer.data(), cells * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(poses_dev, poses_f.data(), poses_f.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("set_path_frame: hipMemcpy failed");
    cilqr_uncertainty_map fm{};
    fm.layer = (const float*)frame_dev_; fm.geom = unc_.geom; fm.poses = poses_dev; fm.layer_stride = 0;
    fm.probes_l = unc_.probes_l; fm.probes_w = unc_.probes_w;
    restore.armed = true;
    check(cilqr_set_uncertainty_map_device(h_, &fm), "cilqr_set_uncertainty_map_device");
  }
  std::vector<double> X(b * 4 * (N + 1)), J(B), total;
  std::vector<int32_t> iters(B), status(B);
  check(cilqr_solve_batch_obstacles(h_, B, N, M, x0.data(), U.data(), poly.data(), fl.data(), M ? &obs_f : nullptr, X.data(), J.data(),
                                    iters.data(), status.data(), CILQR_FLAG_NONE), "cilqr_solve_batch_obstacles");
  if (!step) clear_candidate_fields();
  std::vector<double> scores;
  if (!step && m.min_total) {
    scores.resize(b * CILQR_SCORE_FIELDS);
    total.resize(B);
    check(cilqr_score_batch(h_, B, N, M, X.data(), U.data(), poly.data(), fl.data(), M ? &obs_f : nullptr, max_collision_, scores.data(),
                            total.data()), "cilqr_score_batch");
    last_scores = scores;
  }
  last_frames = frames;
  last_frame_info = info;
  const std::vector<double>& rank = !step && m.min_total ? total : J;
  int best = 0;
  bool have = step;
  if (!step)
    for (int c = 0; c < B; ++c)
      if (rank[c] == rank[c] && (!have || rank[c] < rank[best])) { best = c; have = true; }
  if (!step && m.min_total && !have) return -1;
  // the pick's states and fitted slice back in the map frame
  const double* f = &frames[(size_t)best * CILQR_FRAME_DOUBLES];
  Solved s;
  s.X = Matrix(4, N + 1);
  check(cilqr_frame_states(h_, 1, 1, N, f, 0, CILQR_FRAME_FROM, &X[(size_t)best * 4 * (N + 1)], s.X.a.data()), "cilqr_frame_states");
  s.U.assign(&U[(size_t)best * 2 * N], &U[(size_t)best * 2 * N] + 2 * N);
  s.J = J[best]; s.iters = iters[best]; s.status = status[best];
  install(s, control_seq_);
  const int n = n_ref[best];
  ref_traj_result = Matrix(2, n);
  for (int i = 0; i < n; ++i) {  // (the header's out-of-frame order, on the host: a 2 × n matrix has no heading column to carry)
    const double xf = ref[((size_t)best * W + i) * 2], yf = ref[((size_t)best * W + i) * 2 + 1];
    const double a = f[2] * xf, bb = f[3] * yf, c2 = f[3] * xf, d = f[2] * yf;
    const double rx = a - bb, ry = c2 + d;
    ref_traj_result(0, i) = rx + f[0];
    ref_traj_result(1, i) = ry + f[1];
  }
  return best;
}

void iLQR::set_obstacle_samples(const std::vector<double>& offsets, int n_samples) {
  if (offsets.empty()) {
    samples_.clear();
    n_samples_ = 0;
  } else {
    if (n_samples < 2 || offsets.size() % ((size_t)3 * n_samples) != 0)
      throw std::runtime_error("set_obstacle_samples: needs n_samples >= 2 and n_obs * n_samples * 3 offsets");
    if (offsets.size() / 3 > (size_t)max_obstacles_) throw std::runtime_error("set_obstacle_samples: n_obs * n_samples above max_obstacles");
    if (cov_.on) throw std::logic_error(kCovarianceWithSamples);
    if (tighten_) throw std::logic_error(kTighteningWithSamples);
    if (map_tighten_) throw std::logic_error(kMapTighteningWithSamples);
    samples_ = offsets;
    n_samples_ = n_samples;
  }
  last_risk.clear();
  last_step_hits.clear();
  reserve_block_if_used();  // (the device block holds other arrays with samples than without)
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
  set_noise(offsets, max_risk, lamb, false);
}

void iLQR::set_pose_noise_check_fused(const std::vector<double>& offsets, double max_risk, double lamb) {
  if (offsets.size() % 4 != 0) throw std::runtime_error("set_pose_noise_check_fused: offsets must hold 4 doubles per sample");
  set_noise(offsets, max_risk, lamb, true);
}

void iLQR::set_noise(const std::vector<double>& offsets, double max_risk, double lamb, bool fused) {
  if (cov_.on && !offsets.empty()) throw std::logic_error(kCovarianceWithNoise);
  if (scov_.on && !offsets.empty()) throw std::logic_error(kSampleCovarianceWithNoise);
  noise_ = offsets;
  max_risk_ = max_risk;
  noise_lamb_ = lamb;
  noise_fused_ = fused;
  last_risk.clear();
  last_step_hits.clear();
  reserve_block_if_used();
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

// Sigma0 == nullptr: off, and Sigma0 and W stay as they are.
void iLQR::CovarianceParams::set(const double* Sigma0, const double* W_, double max_risk_, double lamb_, bool sum_) {
  on = Sigma0 != nullptr;
  has_W = on && W_ != nullptr;
  if (on) memcpy(sigma0, Sigma0, sizeof(sigma0));
  if (has_W) memcpy(W, W_, sizeof(W));
  max_risk = max_risk_;
  lamb = lamb_;
  sum = sum_;
}

bool iLQR::CovarianceParams::same_inputs(const double* Sigma0, const double* W_, double lamb_) const {
  return memcmp(sigma0, Sigma0, sizeof(sigma0)) == 0 && has_W == (W_ != nullptr) && (!has_W || memcmp(W, W_, sizeof(W)) == 0) && lamb == lamb_;
}

const double* iLQR::upload(const Block& d, const CovarianceParams& p, size_t s0_at, size_t W_at) const {
  d.up(s0_at, p.sigma0, 16);
  if (p.has_W) d.up(W_at, p.W, 16);
  return p.has_W ? d + W_at : nullptr;
}

void iLQR::set_footprint_check(double min_clearance, double occ_threshold, double margin, bool unknown_hits, bool on) {
  if (on && (min_clearance != min_clearance || occ_threshold != occ_threshold)) throw std::runtime_error("set_footprint_check: min_clearance or occ_threshold is NaN");
  if (on && !(margin >= 0.0 && margin <= 1.7e308)) throw std::runtime_error("set_footprint_check: margin is negative or not finite");
  fp_check_ = on;
  fp_min_clearance_ = min_clearance;
  fp_threshold_ = occ_threshold;
  fp_margin_ = margin;
  fp_unknown_hits_ = unknown_hits;
  last_footprint.clear();
  last_footprint_clearance.clear();
  reserve_block_if_used();  // (the device block holds the check's rows while it is on)
}

void iLQR::set_stop_fallback(const std::vector<double>& decels, int hold, double max_deviation, bool on) {
  if (on) {
    if (decels.empty()) throw std::runtime_error("set_stop_fallback: no braking level");
    for (double d : decels)
      if (!(d > 0.0 && d <= -params.acc_min)) throw std::runtime_error("set_stop_fallback: a level is not in (0, -acc_min]");
    if ((int)decels.size() > max_candidates_) throw std::runtime_error("set_stop_fallback: more levels than max_candidates rows");
    if (hold < 0) throw std::runtime_error("set_stop_fallback: hold is negative");
    if (!(max_deviation >= 0.0)) throw std::runtime_error("set_stop_fallback: max_deviation is negative or NaN");
  }
  stop_on_ = on;
  stop_decel_ = on ? decels : std::vector<double>();
  stop_hold_ = hold;
  stop_max_deviation_ = max_deviation;
  last_stop.clear(); last_stop_footprint.clear();
  last_stop_pick = -1; last_stop_level = -1;
  reserve_block_if_used();  // (the device block holds the levels and the stop rows while it is on)
}

void iLQR::set_map_clearance_check(double min_clearance, double reach, double occ_threshold, double margin, bool unknown_seeds, bool on) {
  if (on && (min_clearance != min_clearance || occ_threshold != occ_threshold)) throw std::runtime_error("set_map_clearance_check: min_clearance or occ_threshold is NaN");
  if (on && !(reach >= 0.0 && reach <= 1.7e308)) throw std::runtime_error("set_map_clearance_check: reach is negative or not finite");
  if (on && !(margin >= 0.0 && margin <= 1.7e308)) throw std::runtime_error("set_map_clearance_check: margin is negative or not finite");
  mc_check_ = on;
  mc_min_clearance_ = min_clearance;
  mc_reach_ = reach;
  mc_threshold_ = occ_threshold;
  mc_margin_ = margin;
  mc_unknown_seeds_ = unknown_seeds;
  last_map_clearance.clear();
  last_map_step_clearance.clear();
  reserve_block_if_used();  // (the device block holds the check's rows while it is on)
}

void iLQR::set_pose_covariance_check(const double Sigma0[16], const double* W, double max_risk, double lamb, bool sum_bound) {
  if (Sigma0 && !noise_.empty()) throw std::logic_error(kCovarianceWithNoise);
  if (Sigma0 && n_samples_) throw std::logic_error(kCovarianceWithSamples);
  if (max_risk != max_risk) throw std::runtime_error("set_pose_covariance_check: max_risk is NaN");
  cov_.set(Sigma0, W, max_risk, lamb, sum_bound);
  last_chance_risk.clear();
  last_step_risk.clear();
  reserve_block_if_used();
}

void iLQR::set_sample_covariance_check(const double Sigma0[16], const double* W, double max_risk, double lamb, bool sum_bound) {
  if (Sigma0 && !noise_.empty()) throw std::logic_error(kSampleCovarianceWithNoise);
  if (max_risk != max_risk) throw std::runtime_error("set_sample_covariance_check: max_risk is NaN");
  scov_.set(Sigma0, W, max_risk, lamb, sum_bound);
  last_chance_risk_sampled.clear();
  reserve_block_if_used();
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
  reserve_block_if_used();  // (the device block holds Sigma_t and the nodes while this check is on)
}

void iLQR::set_chance_tightening(const double Sigma0[16], const double* W, double eps, int rounds, double max_inflate, double lamb) {
  const bool on = Sigma0 != nullptr && rounds != 0;
  if (on && n_samples_) throw std::logic_error(kTighteningWithSamples);
  const double kappa = tightening_kappa("set_chance_tightening", on, eps, rounds, max_inflate);
  if (on) check_tightening_agrees(map_tighten_, mt_rounds_, Sigma0, W, lamb, rounds);
  tighten_ = on;
  // (Sigma0, W and lamb are the one set both tightenings read; switched off, a map tightening keeps them as they are)
  if (on) tg_.set(Sigma0, W, 1.0, lamb, false);
  else if (!map_tighten_) tg_.has_W = false;
  tg_kappa_ = kappa;
  tg_rounds_ = on ? rounds : 0;
  tg_cap_ = max_inflate;
  last_tighten.clear();
  last_tighten_risk_before.clear();
  reserve_block_if_used();
}

// What both tightening setters check of their arguments; kappa, 0 when off.
double iLQR::tightening_kappa(const char* setter, bool on, double eps, int rounds, double max_inflate) const {
  const std::string name = setter;
  if (on && rounds < 0) throw std::runtime_error(name + ": rounds is negative");
  const double kappa = on ? cilqr_chance_kappa(eps) : 0.0;
  if (kappa != kappa) throw std::runtime_error(name + ": eps outside (0, 0.5]");
  if (on && !(max_inflate >= 0.0 && max_inflate <= 1.7e308)) throw std::runtime_error(name + ": max_inflate is negative or not finite");
  return kappa;
}

void iLQR::check_tightening_agrees(bool other_on, int other_rounds, const double Sigma0[16], const double* W, double lamb, int rounds) const {
  if (other_on && !(tg_.same_inputs(Sigma0, W, lamb) && other_rounds == rounds)) throw std::logic_error(kTighteningsDisagree);
}

void iLQR::set_map_tightening(const double Sigma0[16], const double* W, double eps, int rounds, double max_inflate, double lamb) {
  const bool on = Sigma0 != nullptr && rounds != 0;
  if (on && n_samples_) throw std::logic_error(kMapTighteningWithSamples);
  const double kappa = tightening_kappa("set_map_tightening", on, eps, rounds, max_inflate);
  if (on) check_tightening_agrees(tighten_, tg_rounds_, Sigma0, W, lamb, rounds);
  const bool was = map_tighten_;
  map_tighten_ = on;
  if (on) tg_.set(Sigma0, W, 1.0, lamb, false);  // (Sigma0, W and lamb are the one set both tightenings read)
  mt_kappa_ = kappa;
  mt_rounds_ = on ? rounds : 0;
  mt_cap_ = max_inflate;
  last_tighten_map.clear();
  last_tighten_map_risk_before.clear();
  if (map_set_ && (was != on || map_in_block())) apply_map(unc_);  // the layer moves to this object's device block, or back to the handle's
  reserve_block_if_used();
}

void iLQR::set_track_map(double inflate, double z_max, int window, int rounds, bool ellipses) {
  if (rounds < 0 || window < 0 || !(inflate >= 0.0 && inflate <= 1.7e308) || !(z_max >= 0.0 && z_max <= 1.7e308))
    throw std::runtime_error("set_track_map: rounds and window must not be negative, inflate and z_max neither negative nor not finite");
  const bool was = map_in_block();
  tm_rounds_ = rounds; tm_window_ = window; tm_inflate_ = inflate; tm_z_max_ = z_max; tm_ellipses_ = ellipses;
  last_track_map.clear();
  if (map_set_ && (was != map_in_block() || map_in_block())) apply_map(unc_);  // the layer moves to this object's device block, or back
  reserve_block_if_used();
}

// Before anything is enqueued: what a run under set_track_map cannot be combined with.
void iLQR::check_track_map_conflicts() const {
  const CandidateModes m = modes();
  if (!m.track_rounds()) return;
  if (n_samples_) throw std::logic_error(kTrackMapWithSamples);
  if (m.obstacle_rounds() && !tm_ellipses_) throw std::logic_error(kTrackMapEllipsesOffTightened);
  if ((m.obstacle_rounds() && tg_rounds_ != tm_rounds_) || (m.map_rounds() && mt_rounds_ != tm_rounds_)) throw std::logic_error(kTrackMapRoundsDisagree);
}

int iLQR::solve_obstacles() const { return modes().track_rounds() && !tm_ellipses_ ? 0 : (int)obstacles_.size(); }

void iLQR::set_obstacle_covariance(const std::vector<double>& cov) {
  if (trk_on_) throw std::logic_error("set_map_tracker: the tracks carry their own covariance: not with set_obstacle_covariance");
  obs_cov_ = cov;
  pack_obstacles();
}

// One device block for max_candidates candidates at the current horizon, laid out by candidate_layout.h for the modes in force; what
// the setters fixed travels here, once: the pose-noise offsets (the covariance check keeps ONE zero offset, the plan itself, for the
// map risk call) and the quadrature nodes.
void iLQR::reserve_block() {
  const CandidateModes m = modes();
  const CandidateLayout& L = layout_ = candidate_layout(m, sizes());
  hip_check(hipSetDevice(device_), "hipSetDevice");
  if (!block_stream_) {
    hipStream_t st;
    hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreateWithFlags");
    block_stream_ = st;
  }
  hip_check(hipStreamSynchronize((hipStream_t)block_stream_), "hipStreamSynchronize");
  if (block_dev_) hip_check(hipFree(block_dev_), "hipFree");
  block_dev_ = nullptr;
  hip_check(hipMalloc(&block_dev_, L.end * sizeof(double)), "hipMalloc");
  double* d = (double*)block_dev_;
  if (m.cov) hip_check(hipMemset(d + L.delta, 0, 4 * sizeof(double)), "hipMemset");
  else if (m.noise) hip_check(hipMemcpy(d + L.delta, noise_.data(), noise_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  if (m.cmap_arrays()) {
    hip_check(hipMemcpy(d + L.qn, cmap_nodes_.data(), cmap_nodes_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy(d + L.qw, cmap_weights_.data(), cmap_weights_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  }
  if (m.stop_fallback) hip_check(hipMemcpy(d + L.stlv, stop_decel_.data(), stop_decel_.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  block_horizon_ = params.horizon;
}

cilqr_obstacles iLQR::upload_obstacles(const Block& d) {
  cilqr_obstacles obs = obstacle_strides();
  d.up(layout_.pose, obs_pose_.data(), obs_pose_.size());
  d.up(layout_.dim, obs_dim_.data(), obs_dim_.size());
  obs.pose = d + layout_.pose;
  obs.dim = d + layout_.dim;
  return obs;
}

// Every run_candidates with a check, a tightening or the track map in force: prologue -> uploads -> solve -> rounds -> the checks, a
// chain in which each takes the total before it as its base (NaN staying NaN) -> cilqr_argmin_device on the last total -> one wait ->
// the pick's arrays -> one wait.  CandidateModes says which stages run; the block was laid out from the same predicates.
int iLQR::run_candidates_in_block(int B, const std::vector<double>& ego_states, const CandidateModes& m) {
  const int N = params.horizon, M = (int)obstacles_.size(), S = (int)sizes().rollouts(m);
  if (m.footprint && m.sampled) throw std::logic_error(kFootprintWithSamples);
  const int D = (int)stop_decel_.size();
  if (m.stop_fallback_check() && B > max_candidates_ / D)
    throw std::runtime_error("run_candidates (stop fallback): more than floor(max_candidates / levels) candidates: the handle holds max_candidates rows");
  if (m.scov) {
    if (!m.sampled) throw std::logic_error(kSampleCovarianceWithoutSamples);
    if (m.noise) throw std::logic_error(kSampleCovarianceWithNoise);
  } else {
    if (m.cov && m.noise) throw std::logic_error(kCovarianceWithNoise);
    if (m.cov && m.sampled) throw std::logic_error(kCovarianceWithSamples);
    if (tighten_ && m.sampled) throw std::logic_error(kTighteningWithSamples);
    if (map_tighten_ && m.sampled) throw std::logic_error(kMapTighteningWithSamples);
    if (m.sampled && !m.fused) throw std::logic_error(kStoredRowsWithSamples);
    check_track_map_conflicts();
  }
  if (block_horizon_ != N) reserve_block();  // (params is public: the horizon may have changed since the setter)
  const Candidates c = plan_candidates(B, ego_states);
  std::vector<double> nom_pose, nom_dim, samp_off;  // (alive until the stream has been waited for)
  const int n_obs = m.sampled ? pack_sampled(B, nom_pose, nom_dim, samp_off) : 0, ns = n_samples_;
  (void)obstacle_strides();  // (packs again when the horizon changed: the size check below reads the packed covariance)
  const bool judge_cov = m.cov && m.cov_judge && M > 0 && !obs_cov_packed_.empty();
  if ((tighten_ || (m.cov && m.cov_judge)) && M && !obs_cov_.empty() && obs_cov_packed_.empty()) throw std::runtime_error(kObstacleCovarianceSize);
  hip_check(hipSetDevice(device_), "hipSetDevice");
  const Block d = block();
  const CandidateLayout& L = layout_;
  d.up(L.x0, ego_states.data(), (size_t)B * 4);
  d.up(L.U, c.U.data(), c.U.size());
  d.up(L.poly, c.poly.data(), c.poly.size());
  d.up(L.fl, c.fl.data(), c.fl.size());
  cilqr_obstacles obs{};
  if (m.sampled) {
    d.up(L.pose, nom_pose.data(), nom_pose.size());
    d.up(L.dim, nom_dim.data(), nom_dim.size());
    d.up(L.soff, samp_off.data(), samp_off.size());
  } else {
    obs = upload_obstacles(d);
  }
  const cilqr_obstacles* po = M ? &obs : nullptr;
  // under set_track_map with ellipses off the SOLVES read no ellipse: the tracks reach them through the map only; every check still sees them
  const int Ms = solve_obstacles();
  const CovarianceParams& cp = m.scov ? scov_ : cov_;
  const double* cW = m.chance() ? upload(d, cp, L.s0, L.W) : nullptr;
  // (the judge counts the obstacles' own covariance when asked to and one is set; its entries lie by the packed obstacles' strides)
  if (judge_cov) d.up(L.ccov, obs_cov_packed_.data(), obs_cov_packed_.size());
  const double w = m.sampled ? sample_weight() : 0.0, lamb = m.noise ? noise_lamb_ : cp.lamb;
  double* const sigma_out = m.scov || m.map_covariance() ? d + L.csig : nullptr;

  int rc = CILQR_OK;
  size_t total_at = L.J;  // each check takes the total before it as its base and leaves its own
  const auto step = [&](bool runs, auto&& call) { if (runs && !rc) rc = call(); };
  const auto stage = [&](bool runs, size_t out, auto&& call) {
    if (runs && !rc) { rc = call(d + total_at, d + out); total_at = out; }
  };
  const auto score = [&](const double*, double* total) {
    return m.sampled ? cilqr_score_batch_sampled_device(h_, d.st, B, N, n_obs, ns, d + L.X, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                        d + L.soff, w, 1.0, d + L.score, total)
                     : cilqr_score_batch_device(h_, d.st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, m.plain() ? max_collision_ : 1.0,
                                                d + L.score, total);
  };
  const size_t score_out = m.plain() ? L.total : L.base;  // (a check behind it reads the nominal totals as its base)
  step(true, [&] {
    return m.sampled ? cilqr_solve_batch_sampled_device(h_, d.st, B, N, n_obs, ns, d + L.x0, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                        d + L.soff, w, d + L.X, d + L.J, d.i32(L.iters), d.i32(L.status), CILQR_FLAG_NONE)
                     : cilqr_solve_batch_obstacles_device(h_, d.st, B, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, Ms ? po : nullptr, d + L.X,
                                                          d + L.J, d.i32(L.iters), d.i32(L.status), CILQR_FLAG_NONE);
  });
  step(m.rounds(), [&] { return tighten_rounds(d, B, po); });
  stage(m.scored() && m.score_before_gains(), score_out, score);
  step(m.gains(), [&] {
    return m.sampled ? cilqr_gains_batch_sampled_device(h_, d.st, B, N, n_obs, ns, d + L.X, d + L.U, d + L.poly, d + L.fl, d + L.pose, d + L.dim,
                                                        d + L.soff, w, lamb, d + L.k, d + L.K, d.i32(L.ok))
                     : cilqr_gains_batch_device(h_, d.st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, lamb, d + L.k, d + L.K, d.i32(L.ok));
  });
  stage(m.scored() && !m.score_before_gains(), score_out, score);
  stage(m.stored_rows_risk(), L.total, [&](const double*, double* total) {  // (ranks by the mean total over its rollouts: no base)
    const int r = cilqr_rollout_batch_device(h_, d.st, B, N, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, d + L.Xr, d + L.Ur);
    return r ? r : cilqr_score_rollouts_device(h_, d.st, B, N, M, S, d + L.Xr, d + L.Ur, d + L.poly, d + L.fl, po, max_risk_, d + L.rows, d + L.risk, total);
  });
  stage(m.fused_risk(), L.total, [&](const double* base, double* total) {
    return cilqr_rollout_risk_device(h_, d.st, B, N, M, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, po, max_risk_, base, d + L.risk,
                                     d.i32(L.hits), total);
  });
  stage(m.fused_sampled_risk(), L.total, [&](const double* base, double* total) {
    return cilqr_rollout_risk_sampled_device(h_, d.st, B, N, n_obs, ns, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, d + L.pose,
                                             d + L.dim, d + L.soff, max_risk_, base, d + L.risk, d.i32(L.hits), total);
  });
  // (under the sample covariance check the chance call runs with M = 0, for every Sigma_t and the steps that are not finite alone)
  stage(m.chance() && !judge_cov, L.total, [&](const double* base, double* total) {
    return cilqr_chance_risk_device(h_, d.st, B, N, m.scov ? 0 : M, d + L.X, d + L.U, d + L.K, d + L.s0, 0, cW, m.scov ? nullptr : po,
                                    cp.sum ? CILQR_CHANCE_BOUND_SUM : 0u, cp.max_risk, base, d + L.crisk, m.scov ? nullptr : d + L.cstep, nullptr,
                                    sigma_out, total);
  });
  stage(m.chance() && judge_cov, L.total, [&](const double* base, double* total) {
    return cilqr_chance_risk_cov_device(h_, d.st, B, N, M, d + L.X, d + L.U, d + L.K, d + L.s0, 0, cW, po, d + L.ccov,
                                        cp.sum ? CILQR_CHANCE_BOUND_SUM : 0u, cp.max_risk, base, d + L.crisk, d + L.cstep, nullptr, sigma_out, total);
  });
  stage(m.chance_sampled(), L.stotal, [&](const double* base, double* total) {
    return cilqr_chance_risk_sampled_device(h_, d.st, B, N, n_obs, ns, d + L.X, d + L.csig, d + L.pose, d + L.dim, d + L.soff,
                                            cp.sum ? CILQR_CHANCE_SAMPLED_BOUND_SUM : 0u, cp.max_risk, base, d + L.srisk, nullptr, nullptr, nullptr, total);
  });
  stage(m.map_covariance(), L.cmtotal, [&](const double* base, double* total) {  // Sigma_t of the chance call placed on the nodes
    return cilqr_chance_risk_map_device(h_, d.st, B, N, (int)cmap_weights_.size(), d + L.X, d + L.csig, d + L.qn, d + L.qw, cmap_threshold_,
                                        (cmap_sum_ ? CILQR_CHANCE_MAP_BOUND_SUM : 0u) | (cmap_unknown_hits_ ? CILQR_CHANCE_MAP_UNKNOWN_HITS : 0u),
                                        cmap_max_risk_, base, d + L.cmrisk, m.scov ? nullptr : d + L.cmstep, nullptr, nullptr, total);
  });
  stage(m.map_rollout_risk(), L.mtotal, [&](const double* base, double* total) {  // the map's say on top of the obstacles'
    return cilqr_rollout_risk_map_device(h_, d.st, B, N, S, d + L.X, d + L.U, d + L.k, d + L.K, d + L.delta, 0, 0.0, map_threshold_,
                                         map_unknown_hits_ ? CILQR_MAP_RISK_UNKNOWN_HITS : 0u, map_max_risk_, base, d + L.mrisk, d.i32(L.mhits),
                                         d.i32(L.munk), total);
  });
  // the last gate: the final plan's rectangle against the ORIGINAL obstacles and the map on the handle (the original: the rounds put it back)
  stage(m.footprint_check(), L.fptotal, [&](const double* base, double* total) {
    return cilqr_footprint_check_device(h_, d.st, B, N, M, 1, d + L.X, po, fp_margin_, fp_min_clearance_, fp_threshold_,
                                        fp_unknown_hits_ ? CILQR_FOOTPRINT_UNKNOWN_HITS : 0u, base, d + L.fprow, d + L.fpstep, nullptr, total);
  });
  // behind it, while a map is set: how far the rectangle stays from the ORIGINAL map's occupied cells (the map half of min_clearance)
  stage(m.map_clearance_check(), L.mctotal, [&](const double* base, double* total) {
    return cilqr_map_clearance_device(h_, d.st, B, N, 1, d + L.X, mc_margin_, mc_threshold_, mc_reach_, mc_min_clearance_,
                                      mc_unknown_seeds_ ? CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS : 0u, base, d + L.mcrow, d + L.mcstep, total);
  });
  step(true, [&] { return cilqr_argmin_device(h_, d.st, B, d + total_at, d + L.pair); });
  // behind the pick, always: the B final plans braked at every level, judged by the same exact gates with S = D, and a second pick
  if (m.stop_fallback_check()) {
    step(true, [&] {
      return cilqr_stop_plans_device(h_, d.st, B, N, D, d + L.X, d + L.U, d + L.stlv, stop_hold_, stop_max_deviation_, d + L.J, 1.0e6, 0u, d + L.stX,
                                     d + L.stU, d + L.stsp, d + L.stcost);
    });
    size_t stop_total = L.stfptotal;
    step(true, [&] {
      return cilqr_footprint_check_device(h_, d.st, B, N, M, D, d + L.stX, po, fp_margin_, fp_min_clearance_, fp_threshold_,
                                          fp_unknown_hits_ ? CILQR_FOOTPRINT_UNKNOWN_HITS : 0u, d + L.stcost, d + L.stfp, nullptr, nullptr, d + L.stfptotal);
    });
    step(m.map_clearance_check(), [&] {
      stop_total = L.stmctotal;
      return cilqr_map_clearance_device(h_, d.st, B, N, D, d + L.stX, mc_margin_, mc_threshold_, mc_reach_, mc_min_clearance_,
                                        mc_unknown_seeds_ ? CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS : 0u, d + L.stfptotal, d + L.stmc, nullptr, d + L.stmctotal);
    });
    step(true, [&] { return cilqr_argmin_device(h_, d.st, B * D, d + stop_total, d + L.stpair); });
  }
  if (rc) {
    const std::string msg = cilqr_last_error();
    (void)hipStreamSynchronize(d.st);
    throw std::runtime_error((m.scov ? "run_candidates (sample covariance check): " : m.plain() && !m.rounds() ? (m.footprint ? "run_candidates (footprint check): " : "run_candidates (map clearance check): ") : m.plain() ? "run_candidates (chance tightening): "
                                                                                                 : "run_candidates (pose-noise check): ") + msg);
  }
  // every last_* vector is reset here; the stages that ran fill theirs
  clear_candidate_fields();
  double pair[2] = {0.0, -1.0};
  d.down(pair, L.pair, sizeof(pair));
  if (m.cov && !m.scov) {
    d.fetch(last_chance_risk, L.crisk, (size_t)B * CILQR_CHANCE_FIELDS);
    d.fetch(last_step_risk, L.cstep, (size_t)B * N);
  }
  if (m.noise) d.fetch(last_risk, L.risk, (size_t)B * (m.sampled ? CILQR_RRS_FIELDS : m.fused ? CILQR_ROLLOUT_RISK_FIELDS : CILQR_RISK_FIELDS));
  std::vector<double> tg_rows;
  if (m.rounds()) fetch_tighten(d, B, tg_rows);
  if (m.scored()) d.fetch(last_scores, L.score, (size_t)B * CILQR_SCORE_FIELDS);
  if (m.fused_check()) d.fetch(last_step_hits, L.hits, (size_t)B * N);
  if (m.chance_sampled()) d.fetch(last_chance_risk_sampled, L.srisk, (size_t)B * CILQR_CRS_FIELDS);
  if (m.map_covariance()) {
    d.fetch(last_chance_map_risk, L.cmrisk, (size_t)B * CILQR_CHANCE_MAP_FIELDS);
    if (!m.scov) d.fetch(last_map_step_risk, L.cmstep, (size_t)B * N);
  }
  if (m.map_rollout_risk()) {
    d.fetch(last_map_risk, L.mrisk, (size_t)B * CILQR_MAP_RISK_FIELDS);
    d.fetch(last_map_step_hits, L.mhits, (size_t)B * N);
    d.fetch(last_map_unknown_hits, L.munk, (size_t)B * N);
  }
  if (m.footprint_check()) {
    d.fetch(last_footprint, L.fprow, (size_t)B * CILQR_FOOTPRINT_FIELDS);
    d.fetch(last_footprint_clearance, L.fpstep, (size_t)B * N);
  }
  if (m.map_clearance_check()) {
    d.fetch(last_map_clearance, L.mcrow, (size_t)B * CILQR_MAP_CLEARANCE_FIELDS);
    d.fetch(last_map_step_clearance, L.mcstep, (size_t)B * N);
  }
  double stop_pair[2] = {0.0, -1.0};
  if (m.stop_fallback_check()) {
    d.down(stop_pair, L.stpair, sizeof(stop_pair));
    d.fetch(last_stop, L.stsp, (size_t)B * D * CILQR_STOP_FIELDS);
    d.fetch(last_stop_footprint, L.stfp, (size_t)B * D * CILQR_FOOTPRINT_FIELDS);
  }
  d.wait();
  if (m.rounds()) keep_tighten_risk(B, tg_rows);
  const int best = (int)pair[1];
  if (m.stop_fallback_check()) last_stop_pick = (int)stop_pair[1];
  if (best < 0 && last_stop_pick >= 0) {  // every candidate rejected, a stop row is clear: publish it; the warm start stays (not a solve)
    const size_t row = (size_t)last_stop_pick;
    Matrix Xs(4, N + 1), Us(2, N);
    d.down(Xs.a.data(), L.stX + row * 4 * ((size_t)N + 1), Xs.a.size() * sizeof(double));
    d.down(Us.a.data(), L.stU + row * 2 * (size_t)N, Us.a.size() * sizeof(double));
    d.wait();
    X_result = Xs;
    U_result = Us;
    last_stop_level = last_stop_pick % D;
    const int cand = last_stop_pick / D;
    ref_traj_result = Matrix(2, c.n_ref[cand]);
    memcpy(ref_traj_result.a.data(), &c.ref[(size_t)cand * 2 * params.num_of_local_wpts], ref_traj_result.a.size() * sizeof(double));
    return cand;
  }
  if (best < 0) return -1;  // every candidate rejected (and no stop row clear): results and warm start stay
  Solved s;
  fetch_solved(d, best, s);
  d.wait();
  install(s, control_seq_);
  ref_traj_result = Matrix(2, c.n_ref[best]);
  memcpy(ref_traj_result.a.data(), &c.ref[(size_t)best * 2 * params.num_of_local_wpts], ref_traj_result.a.size() * sizeof(double));
  return best;
}

// The rounds behind a solve whose arrays lie in the device block: gains and covariance chain of the current plan against the ORIGINAL
// obstacles `po`, the inflated dense table, the re-solve on it from the U the solve before left.  Sigma0, W and obs_cov travel here.
int iLQR::tighten_rounds(const Block& d, int B, const cilqr_obstacles* po) {
  const int N = params.horizon, M = (int)obstacles_.size();
  const CandidateModes m = modes();
  const CandidateLayout& L = layout_;
  const double* tW = m.chain() ? upload(d, tg_, L.ts0, L.tW) : nullptr;
  if (tighten_ && !obs_cov_packed_.empty()) d.up(L.tcov, obs_cov_packed_.data(), obs_cov_packed_.size());
  cilqr_obstacles inflated{};
  inflated.pose = d + L.tpose;
  inflated.dim = d + L.tdim;
  inflated.batch_stride = (int64_t)M * N;
  inflated.obstacle_stride = N;
  inflated.step_stride = 1;
  // with both tightenings on one round serves both and re-solves once (the setters made the two round counts agree); so it is with the
  // track map beside them: rasterise along the plan, tighten the RASTERISED layers, one re-solve
  const bool trk_on = m.track_rounds(), obs_on = m.obstacle_rounds(), map_on = m.map_rounds(), chain = obs_on || map_on;
  const int Ms = solve_obstacles();  // what the solves read
  const cilqr_obstacles* pos = Ms ? po : nullptr;
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
  if (trk_cov) d.up(L.tkcov, obs_cov_packed_.data(), obs_cov_packed_.size());
  int rc = CILQR_OK;
  for (int r = 0; r < rounds && !rc; ++r) {
    if (chain) {
      rc = cilqr_gains_batch_device(h_, d.st, B, N, M, d + L.X, d + L.U, d + L.poly, d + L.fl, po, tg_.lamb, d + L.k, d + L.K, d.i32(L.ok));
      if (!rc) rc = cilqr_chance_risk_device(h_, d.st, B, N, M, d + L.X, d + L.U, d + L.K, d + L.ts0, 0, tW, po, 0u, 1.0,
                                             nullptr, d + L.trisk, nullptr, nullptr, d + L.tsig, nullptr);
    }
    if (!rc && obs_on)
      rc = cilqr_tighten_obstacles_device(h_, d.st, B, N, M, d + L.X, d + L.tsig, po, obs_cov_packed_.empty() ? nullptr : d + L.tcov, tg_kappa_,
                                          tg_cap_, d + L.tpose, d + L.tdim, d + L.tg);
    // the ORIGINAL layer is the one on the handle here: neither the rasterisation nor the inflation compounds over rounds
    if (!rc && trk_on)
      rc = cilqr_rasterize_tracks_device(h_, d.st, B, N, M, d + L.X, po, trk_cov ? d + L.tkcov : nullptr, tm_inflate_, tm_z_max_, tm_window_, 0u,
                                         first_layers, d + L.tkf);
    if (!rc && map_on && trk_on) rc = cilqr_set_uncertainty_map_device(h_, &rastered);  // the tightening reads the rasterised layers
    if (!rc && map_on) rc = cilqr_tighten_map_device(h_, d.st, B, N, d + L.X, d + L.tsig, mt_kappa_, mt_cap_, trk_on ? second_layers : first_layers, d + L.tmg);
    if (!rc && layers_on) rc = cilqr_set_uncertainty_map_device(h_, &layers);
    if (!rc) rc = cilqr_solve_batch_obstacles_device(h_, d.st, B, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, obs_on ? &inflated : pos, d + L.X,
                                                     d + L.J, d.i32(L.iters), d.i32(L.status), CILQR_FLAG_NONE);
    if (layers_on) {  // the original map is back on the handle whatever happened: what follows judges the plan against it
      const int back = cilqr_set_uncertainty_map_device(h_, &original);  // (a success leaves cilqr_last_error as it is)
      if (!rc) rc = back;
    }
  }
  return rc;
}

void iLQR::fetch_tighten(const Block& d, int B, std::vector<double>& risk_rows) {
  const CandidateModes m = modes();
  risk_rows.assign((size_t)B * CILQR_CHANCE_FIELDS, 0.0);
  if (m.map_rounds()) d.fetch(last_tighten_map, layout_.tmg, (size_t)B * CILQR_TIGHTEN_MAP_FIELDS);
  if (m.obstacle_rounds()) d.fetch(last_tighten, layout_.tg, (size_t)B * CILQR_TIGHTEN_FIELDS);
  if (m.track_rounds()) d.fetch(last_track_map, layout_.tkf, (size_t)B * CILQR_TRACK_MAP_FIELDS);
  if (m.chain()) d.down(risk_rows.data(), layout_.trisk, risk_rows.size() * sizeof(double));  // (of the plan the last round started from)
}

void iLQR::keep_tighten_risk(int B, const std::vector<double>& risk_rows) {
  std::vector<double> before(B);
  for (int b = 0; b < B; ++b) before[b] = risk_rows[(size_t)b * CILQR_CHANCE_FIELDS + CILQR_CR_STEP_RISK];
  if (tighten_ && !obstacles_.empty()) last_tighten_risk_before = before;
  if (map_tighten_ && map_set_) last_tighten_map_risk_before = before;
}

// get_optimal_control_seq under a tightening or the track map: the B = 1 solve and its rounds in the device block, one wait.
void iLQR::solve_tightened(const double x_0[4], Matrix& U, const double poly_coeffs[6], const double fl[2]) {
  const int N = params.horizon, M = (int)obstacles_.size();
  check_track_map_conflicts();
  if (n_samples_ && (tighten_ || map_tighten_)) throw std::logic_error(tighten_ ? kTighteningWithSamples : kMapTighteningWithSamples);
  if (block_horizon_ != N) reserve_block();
  (void)obstacle_strides();
  if (tighten_ && M && !obs_cov_.empty() && obs_cov_packed_.empty()) throw std::runtime_error(kObstacleCovarianceSize);
  hip_check(hipSetDevice(device_), "hipSetDevice");
  const Block d = block();
  const CandidateLayout& L = layout_;
  d.up(L.x0, x_0, 4);
  d.up(L.U, U.a.data(), U.a.size());
  d.up(L.poly, poly_coeffs, CILQR_POLY_COEFFS);
  d.up(L.fl, fl, 2);
  const cilqr_obstacles obs = upload_obstacles(d);
  const cilqr_obstacles* po = M ? &obs : nullptr;
  const int Ms = solve_obstacles();  // (ellipses off: the tracks reach the solve through the map only)
  int rc = cilqr_solve_batch_obstacles_device(h_, d.st, 1, N, Ms, d + L.x0, d + L.U, d + L.poly, d + L.fl, Ms ? po : nullptr, d + L.X, d + L.J,
                                              d.i32(L.iters), d.i32(L.status), CILQR_FLAG_NONE);
  const bool tightened = modes().rounds();
  if (!rc && tightened) rc = tighten_rounds(d, 1, po);
  if (rc) {
    const std::string msg = cilqr_last_error();
    (void)hipStreamSynchronize(d.st);
    throw std::runtime_error("run_step (chance tightening): " + msg);
  }
  Solved s;
  std::vector<double> tg_rows;
  clear_round_fields();
  fetch_solved(d, 0, s);
  if (tightened) fetch_tighten(d, 1, tg_rows);
  d.wait();
  if (tightened) keep_tighten_risk(1, tg_rows);
  install(s, U);
}

}  // namespace cilqr_host

