// cilqr_api.cpp — the C-ABI of include/cilqr.h over the HIP kernels.  No CPU fallback: compute entry points
// fail with CILQR_ERR_NO_DEVICE / CILQR_ERR_HIP when the device path is unavailable.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "cilqr_internal.h"

#include "cilqr_handle.h"
#include "costmap_components.hpp"
#include "costmap_movers.hpp"

namespace cilqr {
thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
}  // namespace cilqr

using cilqr::fail;

namespace {

void derive(const cilqr_params& p, cilqr::KParams& k) {
  k.dt = p.timestep;
  k.desired_speed = p.desired_speed;
  k.tolerance = p.tolerance;
  k.w_acc = p.w_acc; k.w_yawrate = p.w_yawrate; k.w_pos = p.w_pos; k.w_vel = p.w_vel; k.w_obstacle = p.w_obstacle;
  k.q1_acc = p.q1_acc; k.q2_acc = p.q2_acc; k.q1_yawrate = p.q1_yawrate; k.q2_yawrate = p.q2_yawrate;
  k.q1_front = p.q1_front; k.q2_front = p.q2_front; k.q1_rear = p.q1_rear; k.q2_rear = p.q2_rear;
  k.acc_max = p.acc_max; k.acc_min = p.acc_min;
  k.yaw_hi = tan(p.steer_angle_max) / p.wheelbase;
  k.yaw_lo = tan(p.steer_angle_min) / p.wheelbase;
  k.half_dt2 = p.timestep * p.timestep / 2.0;
  k.wheelbase = p.wheelbase; k.speed_max = p.speed_max;
  k.t_safe = p.t_safe; k.s_safe_a = p.s_safe_a; k.s_safe_b = p.s_safe_b;
  k.ego_rad = p.ego_rad; k.ego_front = p.ego_front; k.ego_rear = p.ego_rear;
  k.lamb_factor = p.lamb_factor; k.lamb_max = p.lamb_max;
  k.max_iterations = p.max_iterations;
  k.n_samples = p.num_of_local_wpts * 10;
}

int check_sizes(const cilqr_handle* h, int B, int N, int M) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (B < 0 || B > h->max_batch) return fail(CILQR_ERR_ARG, "B=%d outside [0,%d]", B, h->max_batch);
  if (N < 1 || N > h->max_horizon) return fail(CILQR_ERR_ARG, "N=%d outside [1,%d]", N, h->max_horizon);
  if (M < 0 || M > h->max_obstacles) return fail(CILQR_ERR_ARG, "M=%d outside [0,%d]", M, h->max_obstacles);
  return CILQR_OK;
}

// The environment's A/B and test hooks, read once per handle (cilqr_wave_plan.h says what each does).
cilqr::SolveKnobs read_knobs(int simds) {
  const auto on = [](const char* name) { return getenv(name) != nullptr ? 1 : 0; };
  const auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
  cilqr::SolveKnobs k = {};
  k.simds = simds; k.force_g = num("CILQR_FORCE_G", 0);
  k.hint_off = on("CILQR_NO_SCHEDULE_HINT"); k.pair_on = on("CILQR_PAIR_KERNEL"); k.steal_off = on("CILQR_NO_LANE_SHARING"); k.split_off = on("CILQR_NO_SPLIT_KERNEL");
  k.share_off = on("CILQR_NO_SHARE_KERNEL"); k.tab_budget_kb = num("CILQR_LDS_TABLE_KB", 0);
  k.split_w = num("CILQR_SPLIT_W", 0);  // (test hook: 2 or 4 wavefronts per solve)
  if (on("CILQR_SHARE_W")) k.share_w = num("CILQR_SHARE_W", 0) == 3 ? 3 : 2;  // (A/B hook: two or three wavefronts wherever the kernel applies)
  k.share_max = num("CILQR_SHARE_MAX_B", -1);  // (A/B hook: largest batch on the shared-phase-L kernel; -1: by horizon, share_wavefronts)
  return k;
}

// What every solve call takes from its handle and its sizes; the pointers of the call and its obstacle fields are the caller's.
cilqr::SolveArgs handle_args(const cilqr_handle* h, int B, int N, int M, uint32_t flags) {
  cilqr::SolveArgs a = {};
  a.obs_tab = h->d_obs_tab; a.fwd = h->d_ws;  // (fwd: the grouped family's workspace: 42·N + 12 doubles per solve ≥ the 16·(N + 1) needed here; never both at once)
  a.redo = h->d_redo; a.diag = h->diag; a.passes = h->passes; a.unc = h->unc; a.kp = h->kp;
  a.B = B; a.N = N; a.M = M; a.flags = flags;
  return a;
}

template <typename T>
hipError_t dmalloc(T** p, size_t n) {
  *p = nullptr;
  if (n == 0) return hipSuccess;
  return hipMalloc((void**)p, n * sizeof(T));
}

// Staging of the host-pointer costmap calls: grown when a call needs more than any before it.
int grow(float** p, size_t* cap, size_t n) {
  if (n <= *cap) return CILQR_OK;
  if (*p) HIP_TRY(hipFree(*p));
  *p = nullptr; *cap = 0;
  HIP_TRY(dmalloc(p, n));
  *cap = n;
  return CILQR_OK;
}

void set_obstacles(cilqr::SolveArgs& s, int M, const cilqr_obstacles* obs) {
  if (M <= 0) return;
  s.obs_pose = obs->pose; s.obs_dim = obs->dim; s.obs_weight = obs->weight;
  s.obs_bs = obs->batch_stride; s.obs_ms = obs->obstacle_stride; s.obs_ts = obs->step_stride; s.obs_wbs = obs->weight_batch_stride;
}

// What the four sampled forms check first; `name` is the call's, without its _device suffix.
int check_sampled(const cilqr_handle* h, const char* name, int B, int N, int n_obs, int n_samples) {
  if (n_obs < 1 || n_samples < 2) return fail(CILQR_ERR_ARG, "%s: needs n_obs >= 1 and n_samples >= 2", name);
  if ((long)n_obs * n_samples > 1 << 20) return fail(CILQR_ERR_ARG, "%s: n_obs * n_samples too large", name);
  return check_sizes(h, B, N, n_obs * n_samples);  // the equivalent materialised obstacle count
}

}  // namespace

// The one-wavefront-per-solve family with a schedule hint.  A batch of more solves than SIMDs is dispatched in workgroup order,
// and its launch ends when the last workgroup does: a 20-pass solve that starts among the last costs its full length on top of
// everything else (config-2 scenes at B = 4096: 0.91 ms as given, 0.53 ms with the longest solves first; config 3: 3.8 → 2.4 ms,
// tools/schedule_order.py).  Pass counts are not known in advance — but a planner solves nearly the same scenes tick after tick,
// so each call records its solves' pass counts and a small kernel sorts them into the NEXT call's dispatch order (same batch
// size, same stream; otherwise, and in a first call, the order is the identity).  Any order gives the same results: a solve
// depends on nothing but its own inputs.  CILQR_NO_SCHEDULE_HINT in the environment at create switches it off.
static int launch_wave_scheduled(cilqr_handle* h, cilqr::SolveArgs& a, const cilqr::WavePlan& plan, void* stream) {
  a.order = plan.hinted && h->hint_B == a.B && h->hint_stream == stream ? h->d_order : nullptr;
  a.hint_passes = plan.hinted ? h->d_hint_passes : nullptr;
  HIP_TRY(cilqr::launch_solve_wave(a, plan, (hipStream_t)stream));
  if (plan.hinted) {
    HIP_TRY(cilqr::launch_schedule_order(h->d_hint_passes, a.B, h->d_order, (hipStream_t)stream));
    h->hint_B = a.B; h->hint_stream = stream;
  }
  return CILQR_OK;
}

namespace {

// Obstacle strides of cilqr_solve_batch_obstacles*: none negative, obs given when M > 0; *span / *w_span (may be null) receive the
// entries and weights the strides address (0 when M == 0 or there are no weights).
int check_obstacles(int B, int N, int M, const cilqr_obstacles* o, size_t* span, size_t* w_span) {
  if (span) *span = 0;
  if (w_span) *w_span = 0;
  if (M == 0) return CILQR_OK;
  if (!o) return fail(CILQR_ERR_ARG, "cilqr_solve_batch_obstacles: M = %d but obs is null", M);
  if (!o->pose || !o->dim) return fail(CILQR_ERR_ARG, "cilqr_solve_batch_obstacles: M > 0 but obs->pose or obs->dim is null");
  if (o->batch_stride < 0 || o->obstacle_stride < 0 || o->step_stride < 0 || o->weight_batch_stride < 0)
    return fail(CILQR_ERR_ARG, "cilqr_solve_batch_obstacles: negative stride");
  const int64_t lim = (int64_t)1 << 40;  // (keeps every entry index of the kernels far inside 64 bits)
  if (o->batch_stride > lim || o->obstacle_stride > lim || o->step_stride > lim || o->weight_batch_stride > lim)
    return fail(CILQR_ERR_ARG, "cilqr_solve_batch_obstacles: stride beyond 2^40 entries");
  const int64_t b1 = B > 0 ? B - 1 : 0;
  if (span) *span = (size_t)(b1 * o->batch_stride + (int64_t)(M - 1) * o->obstacle_stride + (int64_t)(N - 1) * o->step_stride + 1);
  if (w_span && o->weight) *w_span = (size_t)(b1 * o->weight_batch_stride + M);
  return CILQR_OK;
}

// The solve behind cilqr_solve_batch_device and cilqr_solve_batch_obstacles_device (arguments checked by the caller).
int solve_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* x0, double* U, const double* poly,
                 const double* xplan_fl, const cilqr_obstacles& o, double* X_out, double* J_out, int32_t* iters_out,
                 int32_t* status_out, uint32_t flags) {
  cilqr::SolveArgs a = handle_args(h, B, N, M, flags);
  a.x0 = x0; a.U = U; a.poly = poly; a.xplan_fl = xplan_fl;
  set_obstacles(a, M, &o);
  // one scene for the batch: the kernels that keep their table in the workspace read one table built in front of them
  a.obs_shared = M > 0 && B > 1 && o.batch_stride == 0 && (!a.obs_weight || o.weight_batch_stride == 0) ? 1 : 0;
  a.X_out = X_out; a.J_out = J_out; a.iters_out = iters_out; a.status_out = status_out;
  a.steal = h->knobs.steal_off ? 0 : 1;
  HIP_TRY(hipSetDevice(h->device));
  const int G = cilqr::plan_group_lanes(h->knobs, B, N, M);
  if (G != 64) { HIP_TRY(cilqr::launch_solve_groups(a, G, h->d_ws, (hipStream_t)stream)); return CILQR_OK; }
  const cilqr::WavePlan plan = cilqr::plan_wave(h->knobs, {B, N, M, 0, h->kp.n_samples, flags, h->unc.layer != nullptr, a.obs_shared != 0});
  if (plan.too_large)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_solve_batch: horizon %d needs %zu bytes of LDS per solve (limit %zu)", N, plan.lds_general, cilqr::SOLVE_LDS_MAX);
  return launch_wave_scheduled(h, a, plan, stream);
}

}  // namespace

extern "C" {

int cilqr_abi_version(void) { return CILQR_ABI_VERSION; }

int cilqr_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  int usable = 0;
  for (int d = 0; d < count; ++d) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++usable;
  }
  return usable;
}

const char* cilqr_last_error(void) { return cilqr::g_last_error.c_str(); }

void cilqr_params_default(cilqr_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  // planning / iLQR (I/Parameters.cpp:6-16)
  p->num_of_local_wpts = 20; p->poly_order = 5; p->desired_speed = 5.0;
  p->timestep = 0.1; p->horizon = 40; p->tolerance = 1e-4; p->max_iterations = 20;
  p->num_states = 4; p->num_ctrls = 2;
  // weights (:19-26)
  p->w_acc = 1.0; p->w_yawrate = 4.0; p->w_pos = 0.65; p->w_vel = 3.0; p->w_obstacle = 1.0; p->w_uncertainty = 1.0;
  // barrier constants (:29-42)
  p->q1_acc = 1.0; p->q2_acc = 1.0; p->q1_yawrate = 1.0; p->q2_yawrate = 1.0;
  p->q1_front = 2.75; p->q2_front = 2.75; p->q1_rear = 2.5; p->q2_rear = 2.5;
  p->q1_uncertainty = 2.5; p->q2_uncertainty = 2.5;
  // limits and vehicle (:45-60)
  p->acc_max = 2.0; p->acc_min = -5.5; p->steer_angle_min = -0.75; p->steer_angle_max = 0.75;
  p->wheelbase = 2.94; p->speed_max = 30.0;
  p->steer_control_max = 1.0; p->steer_control_min = -1.0;
  p->throttle_control_max = 1.0; p->throttle_control_min = -1.0;
  // obstacle model (:63-74)
  p->t_safe = 0.1; p->s_safe_a = 0; p->s_safe_b = 0; p->ego_rad = 1.35;
  p->ego_front = 1.47 + 0.925; p->ego_rear = 1.47 + 0.925;
  p->length = 4.79; p->width = 2.16; p->safe_length = 0.0; p->safe_width = 0.0;
  // I/iLQR.cpp:17-18
  p->lamb_factor = 10; p->lamb_max = 10000;
}

int cilqr_default_control_seq(int N, double* U) {
  if (N < 1 || !U) return fail(CILQR_ERR_ARG, "cilqr_default_control_seq: bad argument");
  const int num_zeros = N / 2;  // I/iLQR.cpp:12
  for (int i = 0; i < N; ++i) {
    U[2 * i] = 0.5;
    U[2 * i + 1] = i < num_zeros ? 0.0 : 0.1;
  }
  return CILQR_OK;
}

int cilqr_create(const cilqr_params* p, int max_batch, int max_horizon, int max_obstacles, int device,
                 cilqr_handle** out) {
  if (!p || !out) return fail(CILQR_ERR_ARG, "cilqr_create: null argument");
  *out = nullptr;
  if (max_batch < 1 || max_horizon < 1 || max_horizon > CILQR_MAX_HORIZON || max_obstacles < 0)
    return fail(CILQR_ERR_ARG, "cilqr_create: sizes out of range (max_horizon ≤ %d)", CILQR_MAX_HORIZON);
  if (p->num_states != CILQR_NX || p->num_ctrls != CILQR_NU || p->poly_order + 1 != CILQR_POLY_COEFFS)
    return fail(CILQR_ERR_UNSUPPORTED, "only num_states=4, num_ctrls=2, poly_order=5 are implemented (reference model, I/Model.cpp)");
  if (p->num_of_local_wpts < 1 || p->num_of_local_wpts > 100 || p->max_iterations < 1)
    return fail(CILQR_ERR_ARG, "cilqr_create: num_of_local_wpts / max_iterations out of range");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(CILQR_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  if (device < 0 || device >= count) return fail(CILQR_ERR_ARG, "device %d not in [0,%d)", device, count);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(CILQR_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(CILQR_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  if (hipSetDevice(device) != hipSuccess) return fail(CILQR_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);

  cilqr_handle* h = new (std::nothrow) cilqr_handle();
  if (!h) return fail(CILQR_ERR_ARG, "out of host memory");
  memset(h, 0, sizeof(*h));
  h->params = *p;
  derive(*p, h->kp);
  h->device = device;
  h->knobs = read_knobs(prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 4 : 1024);
  h->max_batch = max_batch; h->max_horizon = max_horizon; h->max_obstacles = max_obstacles;
  const size_t B = max_batch, N = max_horizon, M = max_obstacles;
  hipError_t err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  // arena and pinned staging of the host-buffer entry points (cilqr_host_io.cpp): calls up to 1 MiB travel packed
  h->arena_cap = cilqr::host_arena_bytes(B, N, M);
  if (err == hipSuccess) err = hipMalloc((void**)&h->d_arena, h->arena_cap);
  h->stage_cap = h->arena_cap < ((size_t)1 << 20) ? h->arena_cap : ((size_t)1 << 20);
  if (err == hipSuccess) err = hipHostMalloc((void**)&h->stage, h->stage_cap, hipHostMallocDefault);
  const size_t Bpad = (B + 63) / 64 * 64;  // the grouped kernels pad the batch to whole wavefronts
  if (err == hipSuccess) err = dmalloc(&h->d_obs_tab, Bpad * M * N * 6);
  if (err == hipSuccess) err = dmalloc(&h->d_ws, cilqr::solve_groups_ws_doubles(max_batch, max_horizon));
  if (err == hipSuccess) err = dmalloc(&h->d_redo, B);
  if (err == hipSuccess) err = dmalloc(&h->d_hint_passes, B);
  if (err == hipSuccess) err = dmalloc(&h->d_order, B);
  h->hint_B = 0; h->hint_stream = nullptr;
  if (err == hipSuccess) err = dmalloc(&h->d_pair, (size_t)2);
  // partial records of cilqr_rollout_risk: max_batch of 8 doubles + max_horizon int32 each
  h->risk_part_stride = cilqr::RISK_PART_DOUBLES + (N + 1) / 2;
  if (err == hipSuccess) err = dmalloc(&h->d_risk_part, B * h->risk_part_stride);
  if (err == hipSuccess) err = dmalloc(&h->d_chance_map_steps, 3 * B * N);
  if (err == hipSuccess) err = dmalloc(&h->d_chance_sampled_steps, cilqr::CHANCE_SAMPLED_REC * B * N);
  if (err == hipSuccess) err = dmalloc(&h->d_footprint_steps, cilqr::footprint_scratch_doubles(B, N));
  if (err == hipSuccess) err = dmalloc(&h->d_tighten_map_part, (size_t)cilqr::TIGHTEN_MAP_REC * cilqr::TIGHTEN_MAP_MAX_G * B);
  if (err == hipSuccess) err = dmalloc(&h->d_track_map_rec, (size_t)cilqr::TRACK_MAP_ENTRY * B * M * N);
  if (err == hipSuccess) err = dmalloc(&h->d_track_map_part, (size_t)cilqr::TRACK_MAP_REC * cilqr::TRACK_MAP_MAX_G * B);
  if (err == hipSuccess) err = dmalloc(&h->d_triple, (size_t)3);
  if (err == hipSuccess) err = dmalloc(&h->d_gather, (size_t)3);
  h->comm_ranks = 1;
  if (err == hipSuccess) err = dmalloc(&h->d_oob, (size_t)1);
  if (err == hipSuccess) err = dmalloc(&h->d_poses, (size_t)8 * 1024 * 4);
  if (err == hipSuccess) err = dmalloc(&h->d_polys, (size_t)8 * cilqr::POLYGON_TABLE_DOUBLES);
  if (err == hipSuccess) err = dmalloc(&h->d_occ_steps, (size_t)8 * 128);
  if (err == hipSuccess) {  // scratch of cilqr_local_plan_batch for max_batch candidates and a 1024-waypoint path
    void* unused = nullptr;
    const size_t W = (size_t)p->num_of_local_wpts;
    if (cilqr::scratch_bytes(h, cilqr::SCR_PLAN_IO, (B * (4 + CILQR_POLY_COEFFS + 2 + 2 * W)) * sizeof(double) + B * sizeof(int32_t), &unused) != CILQR_OK ||
        cilqr::scratch_bytes(h, cilqr::SCR_PLAN_PATH, 2 * 1024 * sizeof(double), &unused) != CILQR_OK)
      err = hipErrorOutOfMemory;
  }
  if (err != hipSuccess) {
    int rc = fail(CILQR_ERR_HIP, "cilqr_create: device allocation failed: %s", hipGetErrorString(err));
    cilqr_destroy(h);
    return rc;
  }
  *out = h;
  return CILQR_OK;
}

int cilqr_destroy(cilqr_handle* h) {
  if (!h) return CILQR_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  (void)cilqr_comm_destroy(h);
  if (h->stage) (void)hipHostFree(h->stage);
  for (void* p : h->scratch)
    if (p) (void)hipFree(p);
  void* ptrs[] = {h->d_poses, h->d_polys, h->d_unc_layer, h->d_triple, h->d_gather, h->d_arena, h->d_obs_tab, h->d_ws, h->d_redo, h->d_hint_passes, h->d_order, h->d_pair, h->d_risk_part, h->d_chance_map_steps, h->d_chance_sampled_steps, h->d_footprint_steps, h->d_tighten_map_part, h->d_track_map_rec, h->d_track_map_part, h->d_src, h->d_dst, h->d_bbox, h->d_oob, h->d_occ_steps};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return CILQR_OK;
}

int cilqr_set_diag_buffer(cilqr_handle* h, uint64_t* dev_buf) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  h->diag = (unsigned long long*)dev_buf;
  return CILQR_OK;
}

namespace {
// include/cilqr.h, cilqr_set_uncertainty_map: geometry and footprint constants of the map cost, formed once on the host
int fill_unc(const cilqr_handle* h, const cilqr_uncertainty_map* m, cilqr::UncArgs& u) {
  if (!m || !m->layer) return fail(CILQR_ERR_ARG, "cilqr_set_uncertainty_map: null map or layer");
  const cilqr_map_geom& g = m->geom;
  if (g.rows < 2 || g.cols < 2 || !(g.res > 0.0) || !(g.len_x > 0.0) || !(g.len_y > 0.0))
    return fail(CILQR_ERR_ARG, "cilqr_set_uncertainty_map: bad geometry (needs at least 2x2 cells)");
  if (m->probes_l < 1 || m->probes_w < 1 || m->probes_l > 64 || m->probes_w > 64)
    return fail(CILQR_ERR_ARG, "cilqr_set_uncertainty_map: probes_l / probes_w must be in [1, 64]");
  if (m->layer_stride < 0 || (m->layer_stride > 0 && m->layer_stride < (int64_t)g.rows * g.cols))
    return fail(CILQR_ERR_ARG, "cilqr_set_uncertainty_map: layer_stride smaller than one layer");
  const cilqr_params& p = h->params;
  u.layer = m->layer;
  u.poses = m->poses;
  u.stride = m->layer_stride;
  u.rows = g.rows; u.cols = g.cols; u.nl = m->probes_l; u.nw = m->probes_w;
  u.x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res);  // cell (0,0) centre, GridMapMath.cpp:114-127
  u.y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res);
  u.inv_res = 1.0 / g.res;
  u.px = m->pose_x; u.py = m->pose_y;
  u.cp = cos(m->pose_theta);  // host libm, like the warp's pose (M/src/local_costmap.cpp:201-202)
  u.sp = sin(m->pose_theta);
  u.la0 = u.nl > 1 ? -0.5 * p.safe_length : 0.0;
  u.la_step = u.nl > 1 ? p.safe_length / (double)(u.nl - 1) : 0.0;
  u.wb0 = u.nw > 1 ? -0.5 * p.safe_width : 0.0;
  u.wb_step = u.nw > 1 ? p.safe_width / (double)(u.nw - 1) : 0.0;
  u.q1 = p.q1_uncertainty; u.q2 = p.q2_uncertainty;
  u.scale = p.w_uncertainty / (double)(u.nl * u.nw);
  return CILQR_OK;
}
}  // namespace

int cilqr_set_uncertainty_map_device(cilqr_handle* h, const cilqr_uncertainty_map* map) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::UncArgs u;
  int rc = fill_unc(h, map, u);
  if (rc) return rc;
  h->unc = u;
  h->unc_res = map->geom.res;
  return CILQR_OK;
}

int cilqr_set_uncertainty_map(cilqr_handle* h, const cilqr_uncertainty_map* map) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (map && (map->layer_stride != 0 || map->poses))
    return fail(CILQR_ERR_ARG, "cilqr_set_uncertainty_map: the host form takes one shared layer (per-solve layers / poses: use the _device form)");
  cilqr::UncArgs u;
  int rc = fill_unc(h, map, u);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)map->geom.rows * map->geom.cols;
  if (n > h->unc_layer_cap) {  // grows on the first tick of a larger map only
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->d_unc_layer) HIP_TRY(hipFree(h->d_unc_layer));
    h->d_unc_layer = nullptr; h->unc_layer_cap = 0;
    HIP_TRY(dmalloc(&h->d_unc_layer, n));
    h->unc_layer_cap = n;
  }
  // on the handle's stream: ordered before the solves of the host-buffer entry points, which use the same stream
  HIP_TRY(hipMemcpyAsync(h->d_unc_layer, map->layer, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // the caller's buffer is free again, and device-pointer solves on other streams see the layer
  u.layer = h->d_unc_layer;
  h->unc = u;
  h->unc_res = map->geom.res;
  return CILQR_OK;
}

int cilqr_clear_uncertainty_map(cilqr_handle* h) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  memset(&h->unc, 0, sizeof(h->unc));
  h->unc_res = 0.0;
  return CILQR_OK;
}

int cilqr_debug_uncertainty_cost(cilqr_handle* h, int n, const double* states, double* cost, double* vx, double* mx) {
  if (!h || n < 1 || !states || !cost || !vx || !mx) return fail(CILQR_ERR_ARG, "cilqr_debug_uncertainty_cost: bad argument");
  if (!h->unc.layer) return fail(CILQR_ERR_ARG, "cilqr_debug_uncertainty_cost: no uncertainty map is set");
  HIP_TRY(hipSetDevice(h->device));
  void* v = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_DEBUG, sizeof(double) * 10 * (size_t)n, &v);
  if (rc) return rc;
  double* d = (double*)v;
  HIP_TRY(hipMemcpyAsync(d, states, sizeof(double) * 4 * n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(cilqr::launch_unc_cost(h->unc, n, d, d + 4 * (size_t)n, d + 5 * (size_t)n, d + 7 * (size_t)n, h->stream));
  HIP_TRY(hipMemcpyAsync(cost, d + 4 * (size_t)n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(vx, d + 5 * (size_t)n, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(mx, d + 7 * (size_t)n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CILQR_OK;
}

int cilqr_set_pass_count_buffer(cilqr_handle* h, int32_t* dev_buf) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  h->passes = dev_buf;
  return CILQR_OK;
}

int cilqr_debug_quu_inverse(cilqr_handle* h, int n, const double* Quu, const double* lamb, double* Qinv, int general) {
  if (!h || n < 1 || !Quu || !lamb || !Qinv) return fail(CILQR_ERR_ARG, "cilqr_debug_quu_inverse: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  void* v = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_DEBUG, sizeof(double) * 9 * (size_t)n, &v);
  if (rc) return rc;
  double *dq = (double*)v, *dl = dq + 4 * (size_t)n, *dout = dl + n;
  HIP_TRY(hipMemcpyAsync(dq, Quu, sizeof(double) * 4 * n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(dl, lamb, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(cilqr::launch_quu_inverse(n, dq, dl, dout, general, h->stream));
  HIP_TRY(hipMemcpyAsync(Qinv, dout, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CILQR_OK;
}

int cilqr_debug_closest_sample(cilqr_handle* h, int n, const double* queries, int32_t* out) {
  if (!h || n < 1 || !queries || !out) return fail(CILQR_ERR_ARG, "cilqr_debug_closest_sample: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  void* v = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_DEBUG, (sizeof(double) * 10 + sizeof(int32_t) * 4) * (size_t)n, &v);
  if (rc) return rc;
  double* din = (double*)v;
  int32_t* dout = reinterpret_cast<int32_t*>(din + 10 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(din, queries, sizeof(double) * 10 * n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(cilqr::launch_closest_sample(n, h->kp.n_samples, din, dout, h->stream));
  HIP_TRY(hipMemcpyAsync(out, dout, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CILQR_OK;
}

int cilqr_debug_blur_ellipse(cilqr_handle* h, int n, const double* abc, double* out) {
  if (!h || n < 1 || !abc || !out) return fail(CILQR_ERR_ARG, "cilqr_debug_blur_ellipse: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  void* v = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_DEBUG, sizeof(double) * 6 * (size_t)n, &v);
  if (rc) return rc;
  double *d_in = (double*)v, *d_out = d_in + 3 * (size_t)n;
  HIP_TRY(hipMemcpyAsync(d_in, abc, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(cilqr::launch_blur_ellipse(n, d_in, d_out, h->stream));
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CILQR_OK;
}

int cilqr_debug_math(cilqr_handle* h, int op, int n, int T, const double* in, double* out) {
  if (!h || n < 1 || !in || !out || op < CILQR_MATH_EXP || op > CILQR_MATH_EXP_FAST) return fail(CILQR_ERR_ARG, "cilqr_debug_math: bad argument");
  const bool chain = op == CILQR_MATH_ROTATE;
  if (chain && (T < 1 || T > CILQR_MAX_HORIZON)) return fail(CILQR_ERR_ARG, "cilqr_debug_math: T must lie in 1..CILQR_MAX_HORIZON");
  const size_t n_in = (size_t)n * (chain ? (size_t)T + 1 : 1);
  const size_t n_out = (size_t)n * (chain ? 2 * (size_t)T : op == CILQR_MATH_EXP || op == CILQR_MATH_EXP_FAST ? 1 : 2);
  HIP_TRY(hipSetDevice(h->device));
  void* v = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_DEBUG, sizeof(double) * (n_in + n_out), &v);
  if (rc) return rc;
  double *d_in = (double*)v, *d_out = d_in + n_in;
  HIP_TRY(hipMemcpyAsync(d_in, in, sizeof(double) * n_in, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(cilqr::launch_debug_math(h->kp, op, n, chain ? T : 0, d_in, d_out, h->stream));
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CILQR_OK;
}

int cilqr_wait(cilqr_handle* h) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CILQR_OK;
}

int cilqr_solve_family(const cilqr_handle* h, int B, int N, int M) {
  if (!h || B < 0 || N < 1 || M < 0) return fail(CILQR_ERR_ARG, "cilqr_solve_family: bad argument");
  return cilqr::plan_group_lanes(h->knobs, B, N, M);
}

int cilqr_solve_wavefronts(const cilqr_handle* h, int B, int N, int M) {
  if (!h || B < 0 || N < 1 || M < 0) return fail(CILQR_ERR_ARG, "cilqr_solve_wavefronts: bad argument");
  return cilqr::query_wavefronts(h->knobs, B, N, M, h->kp.n_samples, h->unc.layer != nullptr);
}

int cilqr_solve_sampled_wavefronts(const cilqr_handle* h, int B, int N, int n_obs) {
  if (!h || B < 0 || N < 1 || n_obs < 1) return fail(CILQR_ERR_ARG, "cilqr_solve_sampled_wavefronts: bad argument");
  return cilqr::split_shape_wavefronts(h->knobs, B, N, n_obs);  // (the rule by shape alone: plan_wave's fall-back beyond 64 KiB of LDS is not in it)
}

int cilqr_solve_batch_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* x0, double* U,
                             const double* poly, const double* xplan_fl, const double* obs_pose, const double* obs_dim,
                             const double* obs_weight, double* X_out, double* J_out, int32_t* iters_out,
                             int32_t* status_out, uint32_t flags) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (!x0 || !U || !poly || !xplan_fl || !X_out) return fail(CILQR_ERR_ARG, "cilqr_solve_batch: null required pointer");
  if (M > 0 && (!obs_pose || !obs_dim)) return fail(CILQR_ERR_ARG, "cilqr_solve_batch: M > 0 but obstacle tables are null");
  const cilqr_obstacles o{obs_pose, obs_dim, obs_weight, (int64_t)M * N, N, 1, M};  // the dense layout
  return solve_device(h, stream, B, N, M, x0, U, poly, xplan_fl, o, X_out, J_out, iters_out, status_out, flags);
}

int cilqr_solve_batch_obstacles_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* x0, double* U,
                                       const double* poly, const double* xplan_fl, const cilqr_obstacles* obs, double* X_out,
                                       double* J_out, int32_t* iters_out, int32_t* status_out, uint32_t flags) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, nullptr, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (!x0 || !U || !poly || !xplan_fl || !X_out) return fail(CILQR_ERR_ARG, "cilqr_solve_batch_obstacles: null required pointer");
  const cilqr_obstacles none{nullptr, nullptr, nullptr, 0, 0, 0, 0};
  return solve_device(h, stream, B, N, M, x0, U, poly, xplan_fl, M > 0 ? *obs : none, X_out, J_out, iters_out, status_out, flags);
}

}  // extern "C"

// The host-buffer solve with ordinary obstacles, enqueued (cilqr_handle.h).  The kernels get device J, iters and status arrays
// whether or not the caller asked for them, and h->d_J points at the costs: the exchange step of cilqr_multi_solve_batch reads them.
int cilqr::host_solve_enqueue(cilqr_handle* h, int B, int N, int M, const double* x0, double* U, const double* poly, const double* xplan_fl,
                              const cilqr_obstacles* obs, size_t span, size_t w_span, double* X_out, double* J_out, int32_t* iters_out,
                              int32_t* status_out, uint32_t flags) {
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  const double* no_samples = nullptr;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_solve(p, B, N, M, 0, x0, U, poly, xplan_fl, o, span, w_span, no_samples, X_out, J_out, iters_out, status_out);
  return cilqr::host_enqueue(h, p, [&] {
    const int rc = cilqr_solve_batch_obstacles_device(h, h->stream, B, N, M, x0, U, poly, xplan_fl, M > 0 ? &o : nullptr, X_out, J_out,
                                                      iters_out, status_out, flags);
    if (rc == CILQR_OK) h->d_J = J_out;
    return rc;
  }, true);
}

extern "C" {

int cilqr_solve_batch(cilqr_handle* h, int B, int N, int M, const double* x0, double* U, const double* poly,
                      const double* xplan_fl, const double* obs_pose, const double* obs_dim, const double* obs_weight,
                      double* X_out, double* J_out, int32_t* iters_out, int32_t* status_out, uint32_t flags) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (!x0 || !U || !poly || !xplan_fl || !X_out) return fail(CILQR_ERR_ARG, "cilqr_solve_batch: null required pointer");
  if (M > 0 && (!obs_pose || !obs_dim)) return fail(CILQR_ERR_ARG, "cilqr_solve_batch: M > 0 but obstacle tables are null");
  const cilqr_obstacles o{obs_pose, obs_dim, obs_weight, (int64_t)M * N, N, 1, M};  // the dense layout
  rc = cilqr::host_solve_enqueue(h, B, N, M, x0, U, poly, xplan_fl, &o, (size_t)B * M * N, (size_t)B * M, X_out, J_out, iters_out, status_out, flags);
  return rc ? rc : cilqr::host_finish(h);
}

int cilqr_solve_batch_obstacles(cilqr_handle* h, int B, int N, int M, const double* x0, double* U, const double* poly,
                                const double* xplan_fl, const cilqr_obstacles* obs, double* X_out, double* J_out,
                                int32_t* iters_out, int32_t* status_out, uint32_t flags) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  size_t span = 0, w_span = 0;
  rc = check_obstacles(B, N, M, obs, &span, &w_span);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (!x0 || !U || !poly || !xplan_fl || !X_out) return fail(CILQR_ERR_ARG, "cilqr_solve_batch_obstacles: null required pointer");
  rc = cilqr::host_solve_enqueue(h, B, N, M, x0, U, poly, xplan_fl, obs, span, w_span, X_out, J_out, iters_out, status_out, flags);
  return rc ? rc : cilqr::host_finish(h);
}

int cilqr_solve_batch_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* x0,
                                     double* U, const double* poly, const double* xplan_fl, const double* nom_pose,
                                     const double* nom_dim, const double* sample_offset, double sample_weight, double* X_out,
                                     double* J_out, int32_t* iters_out, int32_t* status_out, uint32_t flags) {
  int rc = check_sampled(h, "cilqr_solve_batch_sampled", B, N, n_obs, n_samples);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (!x0 || !U || !poly || !xplan_fl || !X_out || !nom_pose || !nom_dim || !sample_offset)
    return fail(CILQR_ERR_ARG, "cilqr_solve_batch_sampled: null required pointer");
  const cilqr::WavePlan plan = cilqr::plan_wave(h->knobs, {B, N, n_obs, n_samples, h->kp.n_samples, flags, h->unc.layer != nullptr, false});
  if (plan.too_large)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_solve_batch_sampled: n_obs * n_samples offset records do not fit LDS beside the solve");
  if (cilqr::sampled_tab_doubles(n_obs, N) > (size_t)h->max_obstacles * 6 * (size_t)h->max_horizon)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_solve_batch_sampled: nominal records exceed the obstacle workspace reserved at create");
  cilqr::SolveArgs a = handle_args(h, B, N, n_obs, flags);  // (obs_tab: n_obs·N·8 doubles per solve ≤ the n_obs·n_samples·N·6 reserved for the materialised form)
  a.x0 = x0; a.U = U; a.poly = poly; a.xplan_fl = xplan_fl;
  a.obs_pose = nom_pose; a.obs_dim = nom_dim;
  a.obs_bs = (long long)n_obs * N; a.obs_ms = N; a.obs_ts = 1;  // (sampled_prologue reads them densely)
  a.X_out = X_out; a.J_out = J_out; a.iters_out = iters_out; a.status_out = status_out;
  a.samp_off = sample_offset; a.n_samples = n_samples; a.samp_w = sample_weight;
  HIP_TRY(hipSetDevice(h->device));
  return launch_wave_scheduled(h, a, plan, stream);  // the LDS-resident family at every batch size
}

int cilqr_solve_batch_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* x0, double* U,
                              const double* poly, const double* xplan_fl, const double* nom_pose, const double* nom_dim,
                              const double* sample_offset, double sample_weight, double* X_out, double* J_out,
                              int32_t* iters_out, int32_t* status_out, uint32_t flags) {
  int rc = check_sampled(h, "cilqr_solve_batch_sampled", B, N, n_obs, n_samples);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (!x0 || !U || !poly || !xplan_fl || !X_out || !nom_pose || !nom_dim || !sample_offset)
    return fail(CILQR_ERR_ARG, "cilqr_solve_batch_sampled: null required pointer");
  cilqr_obstacles o{nom_pose, nom_dim, nullptr, 0, 0, 0, 0};  // the dense nominal tables
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_solve(p, B, N, n_obs, n_samples, x0, U, poly, xplan_fl, o, (size_t)B * n_obs * N, 0, sample_offset, X_out, J_out, iters_out, status_out);
  return cilqr::host_call(h, p, [&] {
    const int rc = cilqr_solve_batch_sampled_device(h, h->stream, B, N, n_obs, n_samples, x0, U, poly, xplan_fl, o.pose, o.dim, sample_offset,
                                                    sample_weight, X_out, J_out, iters_out, status_out, flags);
    if (rc == CILQR_OK) h->d_J = J_out;  // where this call's costs lie
    return rc;
  }, true);
}

int cilqr_argmin_device(cilqr_handle* h, void* stream, int B, const double* J, double* out_pair) {
  if (!h || !J || !out_pair || B < 1) return fail(CILQR_ERR_ARG, "cilqr_argmin_device: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_argmin(J, B, out_pair, nullptr, 0.0, (hipStream_t)stream));
  return CILQR_OK;
}

// ---- scoring of solved trajectories (cilqr_score.hip) --------------------------------------------------------------------
namespace {
// What both score calls share: the solve-side fields of the launch, the on-chip budget, the launch.  `a.s` arrives with its
// obstacle fields set by the caller.
int score_device(cilqr_handle* h, void* stream, cilqr::ScoreArgs& a, const double* X, const double* U, const double* poly,
                 const double* xplan_fl, double max_collision, double* score, double* total, int n_counters) {
  cilqr::SolveArgs& s = a.s;
  s.X_out = const_cast<double*>(X);  // read only (cilqr_internal.h, ScoreArgs)
  s.U = const_cast<double*>(U);
  s.poly = poly; s.xplan_fl = xplan_fl;
  a.score = score; a.total = total; a.max_collision = max_collision; a.w_uncertainty = h->params.w_uncertainty;
  if (a.rows < 1) a.rows = 1;  // (the score calls: one row per solve)
  if (cilqr::score_lds_bytes(s.N, h->kp.n_samples, n_counters) > cilqr::SCORE_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_score_batch: %d path samples, horizon %d and %d sample counters do not fit 64 KiB of LDS",
                h->kp.n_samples, s.N, n_counters);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_score(a, (hipStream_t)stream));
  return CILQR_OK;
}
}  // namespace

int cilqr_score_batch_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* poly,
                             const double* xplan_fl, const cilqr_obstacles* obs, double max_collision, double* score, double* total) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, nullptr, nullptr);
  if (rc) return rc;
  if (!X || !U || !poly || !xplan_fl || !score) return fail(CILQR_ERR_ARG, "cilqr_score_batch: null required pointer");
  if ((int64_t)M * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_score_batch: M * N beyond 2^31 entries");
  if (B == 0) return CILQR_OK;
  cilqr::ScoreArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  return score_device(h, stream, a, X, U, poly, xplan_fl, max_collision, score, total, 0);
}

int cilqr_score_batch_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* X,
                                     const double* U, const double* poly, const double* xplan_fl, const double* nom_pose,
                                     const double* nom_dim, const double* sample_offset, double sample_weight, double max_collision,
                                     double* score, double* total) {
  int rc = check_sampled(h, "cilqr_score_batch_sampled", B, N, n_obs, n_samples);
  if (rc) return rc;
  if (!X || !U || !poly || !xplan_fl || !score || !nom_pose || !nom_dim || !sample_offset)
    return fail(CILQR_ERR_ARG, "cilqr_score_batch_sampled: null required pointer");
  if ((int64_t)n_obs * n_samples * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_score_batch_sampled: n_obs * n_samples * N beyond 2^31 entries");
  if (B == 0) return CILQR_OK;
  cilqr::ScoreArgs a = {};
  a.s = handle_args(h, B, N, n_obs, 0);
  a.s.obs_pose = nom_pose; a.s.obs_dim = nom_dim;
  a.s.samp_off = sample_offset; a.s.n_samples = n_samples; a.s.samp_w = sample_weight;
  return score_device(h, stream, a, X, U, poly, xplan_fl, max_collision, score, total, n_obs * N);
}

int cilqr_score_batch(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* poly,
                      const double* xplan_fl, const cilqr_obstacles* obs, double max_collision, double* score, double* total) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  size_t span = 0, w_span = 0;
  rc = check_obstacles(B, N, M, obs, &span, &w_span);
  if (rc) return rc;
  if (!X || !U || !poly || !xplan_fl || !score) return fail(CILQR_ERR_ARG, "cilqr_score_batch: null required pointer");
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  const double* no_samples = nullptr;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_score(p, B, N, M, 0, X, U, poly, xplan_fl, o, span, w_span, no_samples, score, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_score_batch_device(h, h->stream, B, N, M, X, U, poly, xplan_fl, M > 0 ? &o : nullptr, max_collision, score, total);
  });
}

int cilqr_score_batch_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* U,
                              const double* poly, const double* xplan_fl, const double* nom_pose, const double* nom_dim,
                              const double* sample_offset, double sample_weight, double max_collision, double* score, double* total) {
  int rc = check_sampled(h, "cilqr_score_batch_sampled", B, N, n_obs, n_samples);
  if (rc) return rc;
  if (!X || !U || !poly || !xplan_fl || !score || !nom_pose || !nom_dim || !sample_offset)
    return fail(CILQR_ERR_ARG, "cilqr_score_batch_sampled: null required pointer");
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o{nom_pose, nom_dim, nullptr, 0, 0, 0, 0};  // the dense nominal tables
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_score(p, B, N, n_obs, n_samples, X, U, poly, xplan_fl, o, (size_t)B * n_obs * N, 0, sample_offset, score, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_score_batch_sampled_device(h, h->stream, B, N, n_obs, n_samples, X, U, poly, xplan_fl, o.pose, o.dim, sample_offset,
                                            sample_weight, max_collision, score, total);
  });
}

// ---- feedback gains, closed-loop rollouts, collision risk (cilqr_gains.hip, cilqr_rollout.hip, cilqr_score.hip) -----------------
namespace {
bool is_finite(double v) { return v - v == 0.0; }

// Argument checks that need no handle come first, so that they hold without a device.
int gains_check(const cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* poly, const double* xplan_fl,
                const cilqr_obstacles* obs, double lamb, const double* k_out, const double* K_out, size_t* span, size_t* w_span) {
  if (!X || !U || !poly || !xplan_fl || !k_out || !K_out) return fail(CILQR_ERR_ARG, "cilqr_gains_batch: null required pointer");
  if (!is_finite(lamb)) return fail(CILQR_ERR_ARG, "cilqr_gains_batch: lamb is not finite");
  if (M > 0 && obs && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0))
    return fail(CILQR_ERR_ARG, "cilqr_gains_batch: negative stride");
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  return check_obstacles(B, N, M, obs, span, w_span);
}
int rollout_check(const cilqr_handle* h, int B, int N, int S, const double* X, const double* U, const double* k, const double* K,
                  const double* delta, int64_t delta_batch_stride, double k_scale, const double* X_roll, const double* U_roll, bool host) {
  if (!X || !U || !k || !K || !delta || !X_roll || !U_roll) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: null required pointer");
  if (S < 1) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: S = %d, needs S >= 1", S);
  if (delta_batch_stride < 0 || delta_batch_stride > ((int64_t)1 << 30)) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: negative stride (or one beyond 2^30)");
  if (!is_finite(k_scale)) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: k_scale is not finite");
  int rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  if ((int64_t)B * ((S + 63) / 64) > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: B * S beyond 2^31 wavefronts");
  if (host && (int64_t)B * S > h->max_batch) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: B * S = %lld rows above max_batch = %d (host-buffer form)", (long long)B * S, h->max_batch);
  return CILQR_OK;
}
int score_rollouts_check(const cilqr_handle* h, int B, int N, int M, int S, const double* X_roll, const double* U_roll, const double* poly,
                         const double* xplan_fl, const cilqr_obstacles* obs, const double* row_score, const double* risk, bool host,
                         size_t* span, size_t* w_span) {
  if (!X_roll || !U_roll || !poly || !xplan_fl || !row_score || !risk) return fail(CILQR_ERR_ARG, "cilqr_score_rollouts: null required pointer");
  if (S < 1) return fail(CILQR_ERR_ARG, "cilqr_score_rollouts: S = %d, needs S >= 1", S);
  if (M > 0 && obs && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0))
    return fail(CILQR_ERR_ARG, "cilqr_score_rollouts: negative stride");
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, span, w_span);
  if (rc) return rc;
  if ((int64_t)M * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_score_rollouts: M * N beyond 2^31 entries");
  if ((int64_t)B * S > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_score_rollouts: B * S beyond 2^31 rows");
  if (host && (int64_t)B * S > h->max_batch) return fail(CILQR_ERR_ARG, "cilqr_score_rollouts: B * S = %lld rows above max_batch = %d (host-buffer form)", (long long)B * S, h->max_batch);
  return CILQR_OK;
}
}  // namespace

int cilqr_gains_batch_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* poly,
                             const double* xplan_fl, const cilqr_obstacles* obs, double lamb, double* k_out, double* K_out,
                             int32_t* ok_out) {
  int rc = gains_check(h, B, N, M, X, U, poly, xplan_fl, obs, lamb, k_out, K_out, nullptr, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::gains_lds_bytes(N, h->kp.n_samples) > cilqr::GAINS_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_gains_batch: %d path samples and horizon %d do not fit 64 KiB of LDS", h->kp.n_samples, N);
  cilqr::GainsArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  a.s.X_out = const_cast<double*>(X);  // read only (cilqr_internal.h, GainsArgs)
  a.s.U = const_cast<double*>(U);
  a.s.poly = poly; a.s.xplan_fl = xplan_fl;
  a.k_out = k_out; a.K_out = K_out; a.ok_out = ok_out; a.lamb = lamb;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_gains(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_gains_batch(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* poly,
                      const double* xplan_fl, const cilqr_obstacles* obs, double lamb, double* k_out, double* K_out, int32_t* ok_out) {
  size_t span = 0, w_span = 0;
  int rc = gains_check(h, B, N, M, X, U, poly, xplan_fl, obs, lamb, k_out, K_out, &span, &w_span);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_gains(p, B, N, M, X, U, poly, xplan_fl, o, span, w_span, k_out, K_out, ok_out);
  return cilqr::host_call(h, p, [&] {
    return cilqr_gains_batch_device(h, h->stream, B, N, M, X, U, poly, xplan_fl, M > 0 ? &o : nullptr, lamb, k_out, K_out, ok_out);
  });
}

int cilqr_rollout_batch_device(cilqr_handle* h, void* stream, int B, int N, int S, const double* X, const double* U, const double* k,
                               const double* K, const double* delta, int64_t delta_batch_stride, double k_scale, double* X_roll,
                               double* U_roll) {
  int rc = rollout_check(h, B, N, S, X, U, k, K, delta, delta_batch_stride, k_scale, X_roll, U_roll, false);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::rollout_lds_bytes(N) > cilqr::GAINS_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_rollout_batch: horizon %d does not fit 64 KiB of LDS", N);
  cilqr::RolloutArgs a = {};
  a.X = X; a.U = U; a.k = k; a.K = K; a.delta = delta;
  a.delta_bs = (long long)delta_batch_stride * S * 4;
  a.X_roll = X_roll; a.U_roll = U_roll; a.k_scale = k_scale;
  a.B = B; a.N = N; a.S = S; a.kp = h->kp;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_rollout(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_rollout_batch(cilqr_handle* h, int B, int N, int S, const double* X, const double* U, const double* k, const double* K,
                        const double* delta, int64_t delta_batch_stride, double k_scale, double* X_roll, double* U_roll) {
  int rc = rollout_check(h, B, N, S, X, U, k, K, delta, delta_batch_stride, k_scale, X_roll, U_roll, true);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  // (a stride above 1 would address blocks between the solves' sets)
  if (delta_batch_stride > 1) return fail(CILQR_ERR_ARG, "cilqr_rollout_batch: the host-buffer form takes delta_batch_stride 0 or 1");
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_rollout(p, B, N, S, delta_batch_stride == 0 ? 1 : B, X, U, k, K, delta, X_roll, U_roll);
  return cilqr::host_call(h, p, [&] {
    return cilqr_rollout_batch_device(h, h->stream, B, N, S, X, U, k, K, delta, delta_batch_stride, k_scale, X_roll, U_roll);
  });
}

int cilqr_score_rollouts_device(cilqr_handle* h, void* stream, int B, int N, int M, int S, const double* X_roll, const double* U_roll,
                                const double* poly, const double* xplan_fl, const cilqr_obstacles* obs, double max_risk,
                                double* row_score, double* risk, double* total) {
  int rc = score_rollouts_check(h, B, N, M, S, X_roll, U_roll, poly, xplan_fl, obs, row_score, risk, false, nullptr, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::ScoreArgs a = {};
  a.s = handle_args(h, B * S, N, M, 0);  // (B counts the rows of the launch)
  set_obstacles(a.s, M, obs);
  a.rows = S;
  rc = score_device(h, stream, a, X_roll, U_roll, poly, xplan_fl, 1.0, row_score, nullptr, 0);
  if (rc) return rc;
  const cilqr::RiskArgs r{row_score, risk, total, max_risk, B, S};
  HIP_TRY(cilqr::launch_risk(r, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_score_rollouts(cilqr_handle* h, int B, int N, int M, int S, const double* X_roll, const double* U_roll, const double* poly,
                         const double* xplan_fl, const cilqr_obstacles* obs, double max_risk, double* row_score, double* risk,
                         double* total) {
  size_t span = 0, w_span = 0;
  int rc = score_rollouts_check(h, B, N, M, S, X_roll, U_roll, poly, xplan_fl, obs, row_score, risk, true, &span, &w_span);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_score_rollouts(p, B, N, M, S, X_roll, U_roll, poly, xplan_fl, o, span, w_span, row_score, risk, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_score_rollouts_device(h, h->stream, B, N, M, S, X_roll, U_roll, poly, xplan_fl, M > 0 ? &o : nullptr, max_risk, row_score,
                                       risk, total);
  });
}

// ---- fused rollout risk (cilqr_risk.hip) -------------------------------------------------------------------------------------------
namespace {
// What the three fused forms (obstacles, sampled obstacles, map) check alike, in the order each of them checks it; `who` heads the
// messages.  more_missing: one of the form's own required pointers is null; negative_obs_stride: the obstacle form's strides;
// occ_threshold: the map form's, else null.
int rollout_common_check(const char* who, const double* X, const double* U, const double* k, const double* K, const double* delta,
                         const double* risk, bool more_missing, const double* base, const double* total, int S, int64_t delta_batch_stride,
                         bool negative_obs_stride, double k_scale, double max_risk, const double* occ_threshold) {
  if (!X || !U || !k || !K || !delta || !risk || more_missing) return fail(CILQR_ERR_ARG, "%s: null required pointer", who);
  if (total && !base) return fail(CILQR_ERR_ARG, "%s: total needs base", who);
  if (S < 1) return fail(CILQR_ERR_ARG, "%s: S = %d, needs S >= 1", who, S);
  if (delta_batch_stride < 0 || delta_batch_stride > ((int64_t)1 << 30)) return fail(CILQR_ERR_ARG, "%s: negative stride (or one beyond 2^30)", who);
  if (negative_obs_stride) return fail(CILQR_ERR_ARG, "%s: negative stride", who);
  if (k_scale != k_scale || max_risk != max_risk || (occ_threshold && *occ_threshold != *occ_threshold))
    return fail(CILQR_ERR_ARG, "%s: %s is NaN", who, occ_threshold ? "k_scale, occ_threshold or max_risk" : "k_scale or max_risk");
  return CILQR_OK;
}
// The fields of RolloutRiskArgs the three forms fill alike (a.s and the partial records are the form's own).
void fill_rollout_risk(cilqr::RolloutRiskArgs& a, int S, const double* X, const double* U, const double* k, const double* K, const double* delta,
                       int64_t delta_batch_stride, double k_scale, double max_risk, const double* base, double* risk, int32_t* step_hits,
                       double* total) {
  a.X = X; a.U = U; a.k = k; a.K = K; a.delta = delta;
  a.delta_bs = (long long)delta_batch_stride * S * 4;
  a.k_scale = k_scale; a.max_risk = max_risk;
  a.base = base; a.risk = risk; a.step_hits = step_hits; a.total = total;
  a.S = S; a.G = (S + cilqr::RISK_THREADS - 1) / cilqr::RISK_THREADS;
}
int rollout_risk_check(const cilqr_handle* h, int B, int N, int M, int S, const double* X, const double* U, const double* k,
                       const double* K, const double* delta, int64_t delta_batch_stride, double k_scale, const cilqr_obstacles* obs,
                       double max_risk, const double* base, const double* risk, const double* total, size_t* span, size_t* w_span) {
  const bool negative_obs_stride =
      M > 0 && obs && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0);
  int rc = rollout_common_check("cilqr_rollout_risk", X, U, k, K, delta, risk, false, base, total, S, delta_batch_stride, negative_obs_stride,
                                k_scale, max_risk, nullptr);
  if (rc) return rc;
  rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, span, w_span);
  if (rc) return rc;
  const int64_t G = ((int64_t)S + cilqr::RISK_THREADS - 1) / cilqr::RISK_THREADS;
  if ((int64_t)B * G > h->max_batch)
    return fail(CILQR_ERR_ARG, "cilqr_rollout_risk: B * ceil(S/%d) = %lld partial records above max_batch = %d", cilqr::RISK_THREADS,
                (long long)((int64_t)B * G), h->max_batch);
  return CILQR_OK;
}
}  // namespace

int cilqr_rollout_risk_device(cilqr_handle* h, void* stream, int B, int N, int M, int S, const double* X, const double* U,
                              const double* k, const double* K, const double* delta, int64_t delta_batch_stride, double k_scale,
                              const cilqr_obstacles* obs, double max_risk, const double* base, double* risk, int32_t* step_hits,
                              double* total) {
  int rc = rollout_risk_check(h, B, N, M, S, X, U, k, K, delta, delta_batch_stride, k_scale, obs, max_risk, base, risk, total, nullptr, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::rollout_risk_lds_bytes(N, M) > cilqr::RISK_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_rollout_risk: horizon %d with %d obstacles does not fit 64 KiB of LDS", N, M);
  cilqr::RolloutRiskArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  fill_rollout_risk(a, S, X, U, k, K, delta, delta_batch_stride, k_scale, max_risk, base, risk, step_hits, total);
  a.partials = h->d_risk_part; a.part_stride = (long long)h->risk_part_stride;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_rollout_risk(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_rollout_risk(cilqr_handle* h, int B, int N, int M, int S, const double* X, const double* U, const double* k,
                       const double* K, const double* delta, int64_t delta_batch_stride, double k_scale, const cilqr_obstacles* obs,
                       double max_risk, const double* base, double* risk, int32_t* step_hits, double* total) {
  size_t span = 0, w_span = 0;
  int rc = rollout_risk_check(h, B, N, M, S, X, U, k, K, delta, delta_batch_stride, k_scale, obs, max_risk, base, risk, total, &span, &w_span);
  if (rc) return rc;
  // (a stride above 1 would address blocks between the solves' sets)
  if (delta_batch_stride > 1) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk: the host-buffer form takes delta_batch_stride 0 or 1");
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_rollout_risk(p, B, N, M, S, delta_batch_stride == 0 ? 1 : B, X, U, k, K, delta, o, span, base, risk, step_hits, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_rollout_risk_device(h, h->stream, B, N, M, S, X, U, k, K, delta, delta_batch_stride, k_scale, M > 0 ? &o : nullptr, max_risk,
                                     base, risk, step_hits, total);
  });
}

// ---- the compact sampled form of the gains and of the fused rollout risk (cilqr_gains.hip, cilqr_risk_sampled.hip) -------------------
namespace {
int gains_sampled_check(const cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* U, const double* poly,
                        const double* xplan_fl, const double* nom_pose, const double* nom_dim, const double* sample_offset, double lamb,
                        const double* k_out, const double* K_out) {
  if (!X || !U || !poly || !xplan_fl || !k_out || !K_out || !nom_pose || !nom_dim || !sample_offset)
    return fail(CILQR_ERR_ARG, "cilqr_gains_batch_sampled: null required pointer");
  if (!is_finite(lamb)) return fail(CILQR_ERR_ARG, "cilqr_gains_batch_sampled: lamb is not finite");
  return check_sampled(h, "cilqr_gains_batch_sampled", B, N, n_obs, n_samples);
}
int rollout_risk_sampled_check(const cilqr_handle* h, int B, int N, int n_obs, int n_samples, int S, const double* X, const double* U,
                               const double* k, const double* K, const double* delta, int64_t delta_batch_stride, double k_scale,
                               const double* nom_pose, const double* nom_dim, const double* sample_offset, double max_risk,
                               const double* base, const double* risk, const double* total) {
  int rc = rollout_common_check("cilqr_rollout_risk_sampled", X, U, k, K, delta, risk, !nom_pose || !nom_dim || !sample_offset, base, total, S,
                                delta_batch_stride, false, k_scale, max_risk, nullptr);
  if (rc) return rc;
  rc = check_sampled(h, "cilqr_rollout_risk_sampled", B, N, n_obs, n_samples);
  if (rc) return rc;
  // every count the kernels keep in 32 bits: the sum over a solve's rows of a sample count, an entry index m*N + t, the grid
  if ((int64_t)S * n_samples > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_sampled: S * n_samples beyond 2^31 counts");
  if ((int64_t)n_obs * n_samples * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_sampled: n_obs * n_samples * N beyond 2^31 entries");
  const int64_t G = ((int64_t)S + cilqr::RISK_THREADS - 1) / cilqr::RISK_THREADS;
  if ((int64_t)B * G > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_sampled: B * ceil(S/%d) beyond 2^31 workgroups", cilqr::RISK_THREADS);
  // G > 1: the partial records lie in the obstacle workspace reserved at create (no solve kernel runs inside this call)
  const size_t Bpad = ((size_t)h->max_batch + 63) / 64 * 64;
  if (G > 1 && (size_t)B * (size_t)G * cilqr::rollout_risk_sampled_part_doubles(N, n_obs) > Bpad * h->max_obstacles * h->max_horizon * 6)
    return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_sampled: B * ceil(S/%d) = %lld partial records exceed the obstacle workspace reserved at create",
                cilqr::RISK_THREADS, (long long)((int64_t)B * G));
  return CILQR_OK;
}
}  // namespace

int cilqr_gains_batch_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* X,
                                     const double* U, const double* poly, const double* xplan_fl, const double* nom_pose,
                                     const double* nom_dim, const double* sample_offset, double sample_weight, double lamb,
                                     double* k_out, double* K_out, int32_t* ok_out) {
  int rc = gains_sampled_check(h, B, N, n_obs, n_samples, X, U, poly, xplan_fl, nom_pose, nom_dim, sample_offset, lamb, k_out, K_out);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::gains_lds_bytes(N, h->kp.n_samples) > cilqr::GAINS_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_gains_batch_sampled: %d path samples and horizon %d do not fit 64 KiB of LDS", h->kp.n_samples, N);
  cilqr::GainsArgs a = {};
  a.s = handle_args(h, B, N, n_obs, 0);
  a.s.obs_pose = nom_pose; a.s.obs_dim = nom_dim;
  a.s.samp_off = sample_offset; a.s.n_samples = n_samples; a.s.samp_w = sample_weight;
  a.s.X_out = const_cast<double*>(X);  // read only (cilqr_internal.h, GainsArgs)
  a.s.U = const_cast<double*>(U);
  a.s.poly = poly; a.s.xplan_fl = xplan_fl;
  a.k_out = k_out; a.K_out = K_out; a.ok_out = ok_out; a.lamb = lamb;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_gains(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_gains_batch_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* U,
                              const double* poly, const double* xplan_fl, const double* nom_pose, const double* nom_dim,
                              const double* sample_offset, double sample_weight, double lamb, double* k_out, double* K_out,
                              int32_t* ok_out) {
  int rc = gains_sampled_check(h, B, N, n_obs, n_samples, X, U, poly, xplan_fl, nom_pose, nom_dim, sample_offset, lamb, k_out, K_out);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o{nom_pose, nom_dim, nullptr, 0, 0, 0, 0};  // the dense nominal tables
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_gains_sampled(p, B, N, n_obs, n_samples, X, U, poly, xplan_fl, o, sample_offset, k_out, K_out, ok_out);
  return cilqr::host_call(h, p, [&] {
    return cilqr_gains_batch_sampled_device(h, h->stream, B, N, n_obs, n_samples, X, U, poly, xplan_fl, o.pose, o.dim, sample_offset,
                                            sample_weight, lamb, k_out, K_out, ok_out);
  });
}

int cilqr_rollout_risk_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, int S, const double* X,
                                      const double* U, const double* k, const double* K, const double* delta,
                                      int64_t delta_batch_stride, double k_scale, const double* nom_pose, const double* nom_dim,
                                      const double* sample_offset, double max_risk, const double* base, double* risk,
                                      int32_t* step_hits, double* total) {
  int rc = rollout_risk_sampled_check(h, B, N, n_obs, n_samples, S, X, U, k, K, delta, delta_batch_stride, k_scale, nom_pose, nom_dim,
                                      sample_offset, max_risk, base, risk, total);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::rollout_risk_sampled_lds_bytes(N, n_obs, n_samples) > cilqr::RISK_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_rollout_risk_sampled: horizon %d with %d x %d obstacle samples does not fit 64 KiB of LDS", N,
                n_obs, n_samples);
  cilqr::RolloutRiskArgs a = {};
  a.s = handle_args(h, B, N, n_obs, 0);
  a.s.obs_pose = nom_pose; a.s.obs_dim = nom_dim;
  a.s.samp_off = sample_offset; a.s.n_samples = n_samples;
  fill_rollout_risk(a, S, X, U, k, K, delta, delta_batch_stride, k_scale, max_risk, base, risk, step_hits, total);
  a.partials = h->d_obs_tab; a.part_stride = (long long)cilqr::rollout_risk_sampled_part_doubles(N, n_obs);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_rollout_risk_sampled(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_rollout_risk_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, int S, const double* X, const double* U,
                               const double* k, const double* K, const double* delta, int64_t delta_batch_stride, double k_scale,
                               const double* nom_pose, const double* nom_dim, const double* sample_offset, double max_risk,
                               const double* base, double* risk, int32_t* step_hits, double* total) {
  int rc = rollout_risk_sampled_check(h, B, N, n_obs, n_samples, S, X, U, k, K, delta, delta_batch_stride, k_scale, nom_pose, nom_dim,
                                      sample_offset, max_risk, base, risk, total);
  if (rc) return rc;
  // (a stride above 1 would address blocks between the solves' sets)
  if (delta_batch_stride > 1) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_sampled: the host-buffer form takes delta_batch_stride 0 or 1");
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o{nom_pose, nom_dim, nullptr, 0, 0, 0, 0};  // the dense nominal tables
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_rollout_risk_sampled(p, B, N, n_obs, n_samples, S, delta_batch_stride == 0 ? 1 : B, X, U, k, K, delta, o, sample_offset, base,
                                   risk, step_hits, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_rollout_risk_sampled_device(h, h->stream, B, N, n_obs, n_samples, S, X, U, k, K, delta, delta_batch_stride, k_scale, o.pose,
                                             o.dim, sample_offset, max_risk, base, risk, step_hits, total);
  });
}

// ---- map rollout risk (cilqr_risk_map.hip) -------------------------------------------------------------------------------------------
namespace {
int rollout_risk_map_check(const cilqr_handle* h, int B, int N, int S, const double* X, const double* U, const double* k, const double* K,
                           const double* delta, int64_t delta_batch_stride, double k_scale, double occ_threshold, uint32_t flags,
                           double max_risk, const double* base, const double* risk, const double* total) {
  int rc = rollout_common_check("cilqr_rollout_risk_map", X, U, k, K, delta, risk, false, base, total, S, delta_batch_stride, false, k_scale,
                                max_risk, &occ_threshold);
  if (rc) return rc;
  if (flags & ~CILQR_MAP_RISK_UNKNOWN_HITS) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_map: unknown flag bits 0x%x", flags);
  rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  const int64_t G = ((int64_t)S + cilqr::RISK_THREADS - 1) / cilqr::RISK_THREADS;
  if ((int64_t)B * G > h->max_batch)
    return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_map: B * ceil(S/%d) = %lld partial records above max_batch = %d", cilqr::RISK_THREADS,
                (long long)((int64_t)B * G), h->max_batch);
  if (!h->unc.layer) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_map: no uncertainty map is set on the handle");
  return CILQR_OK;
}
}  // namespace

int cilqr_rollout_risk_map_device(cilqr_handle* h, void* stream, int B, int N, int S, const double* X, const double* U, const double* k,
                                  const double* K, const double* delta, int64_t delta_batch_stride, double k_scale, double occ_threshold,
                                  uint32_t flags, double max_risk, const double* base, double* risk, int32_t* step_hits,
                                  int32_t* unknown_hits, double* total) {
  int rc = rollout_risk_map_check(h, B, N, S, X, U, k, K, delta, delta_batch_stride, k_scale, occ_threshold, flags, max_risk, base, risk, total);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::rollout_risk_map_lds_bytes(N) > cilqr::RISK_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_rollout_risk_map: horizon %d does not fit 64 KiB of LDS", N);
  cilqr::MapRiskArgs a = {};
  a.r.s = handle_args(h, B, N, 0, 0);
  fill_rollout_risk(a.r, S, X, U, k, K, delta, delta_batch_stride, k_scale, max_risk, base, risk, step_hits, total);
  a.r.partials = h->d_risk_part; a.r.part_stride = (long long)h->risk_part_stride;
  a.occ_threshold = occ_threshold; a.unknown_hits = unknown_hits; a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_rollout_risk_map(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_rollout_risk_map(cilqr_handle* h, int B, int N, int S, const double* X, const double* U, const double* k, const double* K,
                           const double* delta, int64_t delta_batch_stride, double k_scale, double occ_threshold, uint32_t flags,
                           double max_risk, const double* base, double* risk, int32_t* step_hits, int32_t* unknown_hits, double* total) {
  int rc = rollout_risk_map_check(h, B, N, S, X, U, k, K, delta, delta_batch_stride, k_scale, occ_threshold, flags, max_risk, base, risk, total);
  if (rc) return rc;
  // (a stride above 1 would address blocks between the solves' sets)
  if (delta_batch_stride > 1) return fail(CILQR_ERR_ARG, "cilqr_rollout_risk_map: the host-buffer form takes delta_batch_stride 0 or 1");
  if (B == 0) return CILQR_OK;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_rollout_risk_map(p, B, N, S, delta_batch_stride == 0 ? 1 : B, X, U, k, K, delta, base, risk, step_hits, unknown_hits, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_rollout_risk_map_device(h, h->stream, B, N, S, X, U, k, K, delta, delta_batch_stride, k_scale, occ_threshold, flags, max_risk,
                                         base, risk, step_hits, unknown_hits, total);
  });
}

// ---- analytic pose-noise risk (cilqr_chance.hip) --------------------------------------------------------------------------------------
namespace {
int chance_risk_check(const cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* K, const double* sigma0,
                      int64_t sigma0_batch_stride, const cilqr_obstacles* obs, uint32_t flags, double max_risk, const double* base,
                      const double* risk, const double* total, size_t* span) {
  if (!X || !U || !K || !sigma0 || !risk) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: null required pointer");
  if (total && !base) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: total needs base");
  if (M > 0 && !obs) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: M = %d but obs is null", M);
  if (M > 0 && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0))
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk: negative stride");
  if (sigma0_batch_stride < 0) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: negative stride");
  if (sigma0_batch_stride > 1) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: sigma0_batch_stride is 0 (one shared) or 1 (one per solve)");
  if (max_risk != max_risk) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: max_risk is NaN");
  if (flags & ~CILQR_CHANCE_BOUND_SUM) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: unknown flag bits 0x%x", flags);
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, span, nullptr);
  if (rc) return rc;
  if ((int64_t)M * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_chance_risk: M * N beyond 2^31 entries");
  return CILQR_OK;
}
}  // namespace

namespace {
// cilqr_chance_risk_device (obs_cov null) and cilqr_chance_risk_cov_device
int chance_risk_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* K,
                       const double* sigma0, int64_t sigma0_batch_stride, const double* process_noise, const cilqr_obstacles* obs,
                       const double* obs_cov, uint32_t flags, double max_risk, const double* base, double* risk, double* step_risk,
                       double* entry_p, double* sigma_out, double* total) {
  int rc = chance_risk_check(h, B, N, M, X, U, K, sigma0, sigma0_batch_stride, obs, flags, max_risk, base, risk, total, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::chance_risk_lds_bytes(N, M) > cilqr::CHANCE_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_chance_risk: horizon %d with %d obstacles does not fit 64 KiB of LDS", N, M);
  cilqr::ChanceArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  a.X = X; a.U = U; a.K = K;
  a.sigma0 = sigma0; a.sigma0_bs = (long long)sigma0_batch_stride * 16; a.W = process_noise;
  a.max_risk = max_risk; a.base = base; a.risk = risk; a.step_risk = step_risk; a.entry_p = entry_p; a.sigma_out = sigma_out;
  a.total = total; a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  if (obs_cov && M > 0) {
    cilqr::ChanceCovArgs c;
    static_cast<cilqr::ChanceArgs&>(c) = a;
    c.obs_cov = obs_cov;
    HIP_TRY(cilqr::launch_chance_risk_cov(c, (hipStream_t)stream));
  } else {
    HIP_TRY(cilqr::launch_chance_risk(a, (hipStream_t)stream));
  }
  return CILQR_OK;
}

// cilqr_chance_risk (obs_cov null) and cilqr_chance_risk_cov
int chance_risk_host(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* K, const double* sigma0,
                     int64_t sigma0_batch_stride, const double* process_noise, const cilqr_obstacles* obs, const double* obs_cov,
                     uint32_t flags, double max_risk, const double* base, double* risk, double* step_risk, double* entry_p,
                     double* sigma_out, double* total) {
  size_t span = 0;
  int rc = chance_risk_check(h, B, N, M, X, U, K, sigma0, sigma0_batch_stride, obs, flags, max_risk, base, risk, total, &span);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  cilqr::HostPlan p(h->d_arena);
  if (M == 0) obs_cov = nullptr;
  if (obs_cov)
    cilqr::plan_chance_risk_cov(p, B, N, M, sigma0_batch_stride == 0 ? 1 : B, X, U, K, sigma0, process_noise, o, span, obs_cov, base, risk,
                                step_risk, entry_p, sigma_out, total);
  else
    cilqr::plan_chance_risk(p, B, N, M, sigma0_batch_stride == 0 ? 1 : B, X, U, K, sigma0, process_noise, o, span, base, risk, step_risk,
                            entry_p, sigma_out, total);
  return cilqr::host_call(h, p, [&] {
    return chance_risk_device(h, h->stream, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, M > 0 ? &o : nullptr, obs_cov,
                              flags, max_risk, base, risk, step_risk, entry_p, sigma_out, total);
  });
}
}  // namespace

int cilqr_chance_risk_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* K,
                             const double* sigma0, int64_t sigma0_batch_stride, const double* process_noise,
                             const cilqr_obstacles* obs, uint32_t flags, double max_risk, const double* base, double* risk,
                             double* step_risk, double* entry_p, double* sigma_out, double* total) {
  return chance_risk_device(h, stream, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, obs, nullptr, flags, max_risk, base,
                            risk, step_risk, entry_p, sigma_out, total);
}

int cilqr_chance_risk(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* K, const double* sigma0,
                      int64_t sigma0_batch_stride, const double* process_noise, const cilqr_obstacles* obs, uint32_t flags,
                      double max_risk, const double* base, double* risk, double* step_risk, double* entry_p, double* sigma_out,
                      double* total) {
  return chance_risk_host(h, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, obs, nullptr, flags, max_risk, base, risk,
                          step_risk, entry_p, sigma_out, total);
}

int cilqr_chance_risk_cov_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* K,
                                 const double* sigma0, int64_t sigma0_batch_stride, const double* process_noise,
                                 const cilqr_obstacles* obs, const double* obs_cov, uint32_t flags, double max_risk, const double* base,
                                 double* risk, double* step_risk, double* entry_p, double* sigma_out, double* total) {
  return chance_risk_device(h, stream, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, obs, obs_cov, flags, max_risk, base,
                            risk, step_risk, entry_p, sigma_out, total);
}

int cilqr_chance_risk_cov(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* K, const double* sigma0,
                          int64_t sigma0_batch_stride, const double* process_noise, const cilqr_obstacles* obs, const double* obs_cov,
                          uint32_t flags, double max_risk, const double* base, double* risk, double* step_risk, double* entry_p,
                          double* sigma_out, double* total) {
  return chance_risk_host(h, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, obs, obs_cov, flags, max_risk, base, risk,
                          step_risk, entry_p, sigma_out, total);
}

// ---- tracked obstacles predicted over the horizon (cilqr_predict.hip) -----------------------------------------------------------------
namespace {
int predict_check(const cilqr_handle* h, int T, int N, int M, const double* track, const double* track_dim, const double* pose_out,
                  const double* dim_out) {
  if (!track || !track_dim || !pose_out || !dim_out) return fail(CILQR_ERR_ARG, "cilqr_predict_obstacles: null required pointer");
  if (T < 1 || N < 1 || M < 1) return fail(CILQR_ERR_ARG, "cilqr_predict_obstacles: T = %d, N = %d, M = %d: each must be at least 1", T, N, M);
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (T > h->max_batch) return fail(CILQR_ERR_ARG, "T=%d outside [1,%d]", T, h->max_batch);
  if (N > h->max_horizon) return fail(CILQR_ERR_ARG, "N=%d outside [1,%d]", N, h->max_horizon);
  if (M > h->max_obstacles) return fail(CILQR_ERR_ARG, "M=%d outside [1,%d]", M, h->max_obstacles);
  if ((int64_t)T * M > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_predict_obstacles: T * M beyond 2^31 tracks");
  return CILQR_OK;
}
}  // namespace

int cilqr_predict_obstacles_device(cilqr_handle* h, void* stream, int T, int N, int M, const double* track, const double* track_dim,
                                   const double* track_cov, const double* track_noise, double* pose_out, double* dim_out,
                                   double* cov_out, double* sigma_out) {
  int rc = predict_check(h, T, N, M, track, track_dim, pose_out, dim_out);
  if (rc) return rc;
  if (cilqr::predict_lds_bytes(N) > cilqr::PREDICT_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_predict_obstacles: horizon %d does not fit 64 KiB of LDS", N);
  cilqr::PredictArgs a = {};
  a.track = track; a.track_dim = track_dim; a.track_cov = track_cov; a.noise = track_noise;
  a.pose_out = pose_out; a.dim_out = dim_out; a.cov_out = cov_out; a.sigma_out = sigma_out;
  a.dt = h->kp.dt; a.half_dt2 = h->kp.half_dt2; a.N = N; a.tracks = (long long)T * M;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_predict_obstacles(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_predict_obstacles(cilqr_handle* h, int T, int N, int M, const double* track, const double* track_dim, const double* track_cov,
                            const double* track_noise, double* pose_out, double* dim_out, double* cov_out, double* sigma_out) {
  int rc = predict_check(h, T, N, M, track, track_dim, pose_out, dim_out);
  if (rc) return rc;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_predict_obstacles(p, T, N, M, track, track_dim, track_cov, track_noise, pose_out, dim_out, cov_out, sigma_out);
  return cilqr::host_call(h, p, [&] {
    return cilqr_predict_obstacles_device(h, h->stream, T, N, M, track, track_dim, track_cov, track_noise, pose_out, dim_out, cov_out,
                                          sigma_out);
  });
}

// ---- map obstacles tracked across ticks (cilqr_track.hip) ------------------------------------------------------------------------------
namespace {
int track_update_check(const cilqr_handle* h, int W, int M, int D, const double* det, int64_t n_det_stride, const cilqr_track_filter* f,
                       const double* state_in, const double* state_out, const double* world, uint32_t flags, const double* track_out,
                       const double* dim_out, const double* cov_out) {
  if (!f || !state_out || !world || !track_out || !dim_out || !cov_out)
    return fail(CILQR_ERR_ARG, "cilqr_track_update: null required pointer");
  if (flags & ~CILQR_TRACK_RESET) return fail(CILQR_ERR_ARG, "cilqr_track_update: unknown flag bits 0x%x", flags);
  if (!state_in && !(flags & CILQR_TRACK_RESET)) return fail(CILQR_ERR_ARG, "cilqr_track_update: null state_in without CILQR_TRACK_RESET");
  if (W < 1 || M < 1 || D < 0) return fail(CILQR_ERR_ARG, "cilqr_track_update: W = %d, M = %d, D = %d: W and M must be at least 1, D at least 0", W, M, D);
  if (D > 0 && !det) return fail(CILQR_ERR_ARG, "cilqr_track_update: D = %d but det is null", D);
  if (n_det_stride < 0) return fail(CILQR_ERR_ARG, "cilqr_track_update: negative n_det_stride");
  if (!(f->dt > 0.0 && f->dt <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_track_update: dt is not > 0 or not finite");
  if (!(f->gate2 >= 0.0)) return fail(CILQR_ERR_ARG, "cilqr_track_update: gate2 is negative or NaN");
  if (!(f->v_min >= 0.0)) return fail(CILQR_ERR_ARG, "cilqr_track_update: v_min is negative or NaN");
  if (!(f->theta_var_slow >= 0.0)) return fail(CILQR_ERR_ARG, "cilqr_track_update: theta_var_slow is negative or NaN");
  if (f->min_hits < 1) return fail(CILQR_ERR_ARG, "cilqr_track_update: min_hits = %d, must be at least 1", f->min_hits);
  if (f->max_misses < 0) return fail(CILQR_ERR_ARG, "cilqr_track_update: max_misses = %d is negative", f->max_misses);
  if (M > CILQR_TRACK_MAX_SLOTS || D > CILQR_TRACK_MAX_DETECTIONS)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_track_update: M = %d slots, D = %d detections: at most %d and %d", M, D, CILQR_TRACK_MAX_SLOTS,
                CILQR_TRACK_MAX_DETECTIONS);
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (W > h->max_batch) return fail(CILQR_ERR_ARG, "W=%d outside [1,%d]", W, h->max_batch);
  if (M > h->max_obstacles) return fail(CILQR_ERR_ARG, "M=%d outside [1,%d]", M, h->max_obstacles);
  return CILQR_OK;
}
}  // namespace

int cilqr_track_update_device(cilqr_handle* h, void* stream, int W, int M, int D, const double* det, const int32_t* n_det,
                              int64_t n_det_stride, const cilqr_track_filter* f, const double* state_in, double* state_out,
                              double* world, uint32_t flags, int32_t* assign, double* track_out, double* dim_out, double* cov_out) {
  int rc = track_update_check(h, W, M, D, det, n_det_stride, f, state_in, state_out, world, flags, track_out, dim_out, cov_out);
  if (rc) return rc;
  cilqr::TrackArgs a = {};
  a.det = det; a.n_det = n_det; a.state_in = state_in; a.state_out = state_out; a.world = world; a.assign = assign;
  a.track_out = track_out; a.dim_out = dim_out; a.cov_out = cov_out;
  a.n_det_stride = n_det_stride; a.f = *f; a.W = W; a.M = M; a.D = D; a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_track_update(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_track_update(cilqr_handle* h, int W, int M, int D, const double* det, const int32_t* n_det, int64_t n_det_stride,
                       const cilqr_track_filter* f, const double* state_in, double* state_out, double* world, uint32_t flags,
                       int32_t* assign, double* track_out, double* dim_out, double* cov_out) {
  int rc = track_update_check(h, W, M, D, det, n_det_stride, f, state_in, state_out, world, flags, track_out, dim_out, cov_out);
  if (rc) return rc;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_track_update(p, W, M, D, n_det ? (size_t)(W - 1) * (size_t)n_det_stride + 1 : 0, (flags & CILQR_TRACK_RESET) != 0, det, n_det,
                           state_in, state_out, world, assign, track_out, dim_out, cov_out);
  return cilqr::host_call(h, p, [&] {
    return cilqr_track_update_device(h, h->stream, W, M, D, det, n_det, n_det_stride, f, state_in, state_out, world, flags, assign,
                                     track_out, dim_out, cov_out);
  });
}

// ---- chance-constraint tightening (cilqr_tighten.hip) ---------------------------------------------------------------------------------
namespace {
int tighten_check(const cilqr_handle* h, int B, int N, int M, const double* X, const double* sigma, const cilqr_obstacles* obs,
                  double kappa, double max_inflate, const double* dim_out, const double* tighten, size_t* span) {
  if (!X || !sigma || !dim_out || !tighten) return fail(CILQR_ERR_ARG, "cilqr_tighten_obstacles: null required pointer");
  if (M > 0 && !obs) return fail(CILQR_ERR_ARG, "cilqr_tighten_obstacles: M = %d but obs is null", M);
  if (M > 0 && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0))
    return fail(CILQR_ERR_ARG, "cilqr_tighten_obstacles: negative stride");
  if (!(kappa >= 0.0 && kappa <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_tighten_obstacles: kappa is negative or not finite");
  if (!(max_inflate >= 0.0 && max_inflate <= 1.7e308))
    return fail(CILQR_ERR_ARG, "cilqr_tighten_obstacles: max_inflate is negative or not finite");
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, span, nullptr);
  if (rc) return rc;
  if ((int64_t)M * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_tighten_obstacles: M * N beyond 2^31 entries");
  return CILQR_OK;
}
}  // namespace

namespace {
// (arguments checked by the caller; with M = 0 the host form's dim_out has no place in the arena and is null here)
int tighten_launch(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* sigma, const cilqr_obstacles* obs,
                   const double* obs_cov, double kappa, double max_inflate, double* pose_out, double* dim_out, double* tighten) {
  if (cilqr::tighten_lds_bytes(N) > cilqr::TIGHTEN_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_tighten_obstacles: horizon %d does not fit 64 KiB of LDS", N);
  cilqr::TightenArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  a.X = X; a.sigma = sigma; a.obs_cov = M > 0 ? obs_cov : nullptr;
  a.kappa = kappa; a.max_inflate = max_inflate;
  a.pose_out = M > 0 ? pose_out : nullptr; a.dim_out = dim_out; a.tighten = tighten;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_tighten_obstacles(a, (hipStream_t)stream));
  return CILQR_OK;
}
}  // namespace

int cilqr_tighten_obstacles_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* sigma,
                                   const cilqr_obstacles* obs, const double* obs_cov, double kappa, double max_inflate,
                                   double* pose_out, double* dim_out, double* tighten) {
  int rc = tighten_check(h, B, N, M, X, sigma, obs, kappa, max_inflate, dim_out, tighten, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  return tighten_launch(h, stream, B, N, M, X, sigma, obs, obs_cov, kappa, max_inflate, pose_out, dim_out, tighten);
}

int cilqr_tighten_obstacles(cilqr_handle* h, int B, int N, int M, const double* X, const double* sigma, const cilqr_obstacles* obs,
                            const double* obs_cov, double kappa, double max_inflate, double* pose_out, double* dim_out,
                            double* tighten) {
  size_t span = 0;
  int rc = tighten_check(h, B, N, M, X, sigma, obs, kappa, max_inflate, dim_out, tighten, &span);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  if (M == 0) { obs_cov = nullptr; pose_out = nullptr; }
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_tighten_obstacles(p, B, N, M, X, sigma, o, span, obs_cov, pose_out, dim_out, tighten);
  return cilqr::host_call(h, p, [&] {
    return tighten_launch(h, h->stream, B, N, M, X, sigma, M > 0 ? &o : nullptr, obs_cov, kappa, max_inflate, pose_out, dim_out, tighten);
  });
}

// ---- map tightening (cilqr_tighten_map.hip) --------------------------------------------------------------------------------------------
namespace {
// what needs no handle
int tighten_map_args_check(const double* X, const double* sigma, double kappa, double max_inflate, const float* layer_out,
                           const double* tighten) {
  if (!X || !sigma || !layer_out || !tighten) return fail(CILQR_ERR_ARG, "cilqr_tighten_map: null required pointer");
  if (!(kappa >= 0.0 && kappa <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_tighten_map: kappa is negative or not finite");
  if (!(max_inflate >= 0.0 && max_inflate <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_tighten_map: max_inflate is negative or not finite");
  return CILQR_OK;
}
int tighten_map_handle_check(const cilqr_handle* h, int B, int N) {
  int rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  if (!h->unc.layer) return fail(CILQR_ERR_ARG, "cilqr_tighten_map: no uncertainty map is set on the handle");
  if ((int64_t)h->unc.rows * h->unc.cols > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_tighten_map: the map has 2^31 cells or more");
  return CILQR_OK;
}
}  // namespace

int cilqr_tighten_map_device(cilqr_handle* h, void* stream, int B, int N, const double* X, const double* sigma, double kappa,
                             double max_inflate, float* layer_out, double* tighten) {
  int rc = tighten_map_args_check(X, sigma, kappa, max_inflate, layer_out, tighten);
  if (rc) return rc;
  rc = tighten_map_handle_check(h, B, N);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  const size_t cells = (size_t)h->unc.rows * h->unc.cols;
  {  // the dilation reads neighbours: the output must not be the layer it reads
    const float* in0 = h->unc.layer;
    const float* in1 = in0 + (size_t)(B - 1) * (size_t)h->unc.stride + cells;
    if (layer_out < in1 && in0 < layer_out + (size_t)B * cells)
      return fail(CILQR_ERR_ARG, "cilqr_tighten_map: layer_out overlaps the layer set on the handle");
  }
  if (cilqr::tighten_map_lds_bytes(N) > cilqr::TIGHTEN_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_tighten_map: horizon %d does not fit 64 KiB of LDS", N);
  cilqr::TightenMapArgs a = {};
  a.s = handle_args(h, B, N, 0, 0);
  a.X = X; a.sigma = sigma; a.kappa = kappa; a.max_inflate = max_inflate;
  a.res = h->unc_res;
  a.r_fp = 0.5 * sqrt(h->params.safe_length * h->params.safe_length + h->params.safe_width * h->params.safe_width);
  a.layer_out = layer_out; a.tighten = tighten;
  a.partials = h->d_tighten_map_part;  // (reserved at create: TIGHTEN_MAP_MAX_G records per solve of max_batch)
  const size_t tiles = (cells + cilqr::TIGHTEN_MAP_THREADS - 1) / cilqr::TIGHTEN_MAP_THREADS;
  a.G = (int)(tiles < (size_t)cilqr::TIGHTEN_MAP_MAX_G ? tiles : (size_t)cilqr::TIGHTEN_MAP_MAX_G);
  if ((int64_t)B * a.G > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_tighten_map: B * %d workgroups per solve beyond 2^31 - 1", a.G);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_tighten_map(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_tighten_map(cilqr_handle* h, int B, int N, const double* X, const double* sigma, double kappa, double max_inflate,
                      float* layer_out, double* tighten) {
  int rc = tighten_map_args_check(X, sigma, kappa, max_inflate, layer_out, tighten);
  if (rc) return rc;
  rc = tighten_map_handle_check(h, B, N);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_tighten_map(p, B, N, (size_t)h->unc.rows * h->unc.cols, X, sigma, layer_out, tighten);
  return cilqr::host_call(h, p, [&] { return cilqr_tighten_map_device(h, h->stream, B, N, X, sigma, kappa, max_inflate, layer_out, tighten); });
}

// ---- predicted tracks rasterised into the map along each plan (cilqr_track_map.hip) ---------------------------------------------------
namespace {
// what needs no handle
int track_map_args_check(int B, int N, int M, const cilqr_obstacles* obs, double inflate, double z_max, int window, uint32_t flags,
                         const float* layer_out, const double* fields) {
  if (!obs || !obs->pose || !obs->dim || !layer_out || !fields) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: null required pointer");
  if (B < 1 || N < 1 || M < 1) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: B = %d, N = %d, M = %d: each must be at least 1", B, N, M);
  if (!(inflate >= 0.0 && inflate <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: inflate is negative or not finite");
  if (!(z_max >= 0.0 && z_max <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: z_max is negative or not finite");
  if (window < 0) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: window is negative");
  if (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0)
    return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: negative stride");
  if (flags & ~CILQR_TRACK_MAP_BOUND_MIN) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
int track_map_handle_check(const cilqr_handle* h, int B, int N, int M, const cilqr_obstacles* obs, size_t* span) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, span, nullptr);
  if (rc) return rc;
  if (!h->unc.layer) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: no uncertainty map is set on the handle");
  if ((int64_t)h->unc.rows * h->unc.cols > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: the map has 2^31 cells or more");
  return CILQR_OK;
}
}  // namespace

int cilqr_rasterize_tracks_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const cilqr_obstacles* obs,
                                  const double* obs_cov, double inflate, double z_max, int window, uint32_t flags, float* layer_out,
                                  double* fields) {
  int rc = track_map_args_check(B, N, M, obs, inflate, z_max, window, flags, layer_out, fields);
  if (rc) return rc;
  rc = track_map_handle_check(h, B, N, M, obs, nullptr);
  if (rc) return rc;
  const size_t cells = (size_t)h->unc.rows * h->unc.cols;
  {  // the output must not be the layer the call reads
    const float* in0 = h->unc.layer;
    const float* in1 = in0 + (size_t)(B - 1) * (size_t)h->unc.stride + cells;
    if (layer_out < in1 && in0 < layer_out + (size_t)B * cells)
      return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: layer_out overlaps the layer set on the handle");
  }
  if (cilqr::track_map_lds_bytes(N) > cilqr::TRACK_MAP_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_rasterize_tracks: horizon %d does not fit 64 KiB of LDS", N);
  cilqr::TrackMapArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  a.X = X; a.obs_cov = obs_cov; a.inflate = inflate; a.z_max = z_max; a.res = h->unc_res;
  a.layer_out = layer_out; a.fields = fields;
  a.records = h->d_track_map_rec;    // (reserved at create: max_batch sets of max_obstacles·max_horizon records)
  a.partials = h->d_track_map_part;  // (reserved at create: TRACK_MAP_MAX_G records per solve of max_batch)
  const size_t tiles = (cells + cilqr::TRACK_MAP_THREADS - 1) / cilqr::TRACK_MAP_THREADS;
  a.G = (int)(tiles < (size_t)cilqr::TRACK_MAP_MAX_G ? tiles : (size_t)cilqr::TRACK_MAP_MAX_G);
  a.window = window < N ? window : N;  // (beyond N - 1 every step takes part: the sums of the kernel stay inside an int)
  a.sets = obs->batch_stride == 0 ? 1 : B;
  a.flags = flags;
  const int64_t chunks = ((int64_t)M * N + cilqr::TRACK_MAP_THREADS - 1) / cilqr::TRACK_MAP_THREADS;
  if ((int64_t)B * a.G > 0x7fffffff || (int64_t)a.sets * chunks > 0x7fffffff || (int64_t)M * N > 0x7fffffff)
    return fail(CILQR_ERR_ARG, "cilqr_rasterize_tracks: B * %d workgroups per solve, or the entries' workgroups, beyond 2^31 - 1", a.G);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_rasterize_tracks(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_rasterize_tracks(cilqr_handle* h, int B, int N, int M, const double* X, const cilqr_obstacles* obs, const double* obs_cov,
                           double inflate, double z_max, int window, uint32_t flags, float* layer_out, double* fields) {
  int rc = track_map_args_check(B, N, M, obs, inflate, z_max, window, flags, layer_out, fields);
  if (rc) return rc;
  size_t span = 0;
  rc = track_map_handle_check(h, B, N, M, obs, &span);
  if (rc) return rc;
  cilqr_obstacles o = *obs;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_rasterize_tracks(p, B, N, (size_t)h->unc.rows * h->unc.cols, X, o, span, obs_cov, layer_out, fields);
  return cilqr::host_call(h, p, [&] {
    return cilqr_rasterize_tracks_device(h, h->stream, B, N, M, X, &o, obs_cov, inflate, z_max, window, flags, layer_out, fields);
  });
}

// ---- analytic map risk (cilqr_chance_map.hip) ------------------------------------------------------------------------------------------
namespace {
// what needs no handle
int chance_map_args_check(int Q, const double* X, const double* sigma, const double* nodes, const double* weights, double occ_threshold,
                          uint32_t flags, double max_risk, const double* base, const double* risk, const double* total) {
  if (!X || !sigma || !nodes || !weights || !risk) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: null required pointer");
  if (total && !base) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: total needs base");
  if (Q < 1 || Q > CILQR_MAX_QUAD_NODES)
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: Q = %d outside [1, %d]", Q, CILQR_MAX_QUAD_NODES);
  if (occ_threshold != occ_threshold || max_risk != max_risk)
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: occ_threshold or max_risk is NaN");
  if (flags & ~(CILQR_CHANCE_MAP_UNKNOWN_HITS | CILQR_CHANCE_MAP_BOUND_SUM))
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
int chance_map_handle_check(const cilqr_handle* h, int B, int N) {
  int rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  if (!h->unc.layer) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: no uncertainty map is set on the handle");
  return CILQR_OK;
}

// He_n(x) and He_(n-1)(x) by the recurrence He_(k+1) = x He_k - k He_(k-1)
void hermite_e(int n, double x, double* he_n, double* he_n1) {
  double a = 1.0, b = 0.0;  // He_0, "He_-1"
  for (int k = 0; k < n; ++k) {
    const double c = x * a - (double)k * b;
    b = a; a = c;
  }
  *he_n = a; *he_n1 = b;
}
// The n nodes (ascending) and weights of the probabilists' Gauss-Hermite rule, weights summing to 1.
void gauss_hermite_e(int n, double* z, double* w) {
  double prev[10], cur[10];
  int m_prev = 0;
  for (int m = 1; m <= n; ++m) {  // the roots of He_m from the brackets the roots of He_(m-1) give
    const double bound = 2.0 * sqrt((double)m) + 1.0;  // beyond the largest root (< 2 sqrt m)
    for (int i = 0; i < m; ++i) {
      double lo = i == 0 ? -bound : prev[i - 1], hi = i == m_prev ? bound : prev[i];
      double f_lo, d;
      hermite_e(m, lo, &f_lo, &d);
      double x = 0.5 * (lo + hi);
      for (int it = 0; it < 100; ++it) {
        double f, f1;
        hermite_e(m, x, &f, &f1);
        if (f == 0.0) break;
        if ((f < 0.0) == (f_lo < 0.0)) lo = x; else hi = x;
        double nx = x - f / ((double)m * f1);  // He_m' = m He_(m-1)
        if (!(nx > lo && nx < hi)) nx = 0.5 * (lo + hi);  // (a step that leaves the bracket: bisect)
        if (nx == x) break;
        x = nx;
      }
      cur[i] = x;
    }
    for (int i = 0; i < m; ++i) prev[i] = cur[i];
    m_prev = m;
  }
  for (int i = 0; i < n / 2; ++i) {  // mirrored about 0
    const double r = 0.5 * (prev[n - 1 - i] - prev[i]);
    prev[i] = -r; prev[n - 1 - i] = r;
  }
  if (n & 1) prev[n / 2] = 0.0;
  double fact = 1.0, sum = 0.0;
  for (int k = 2; k < n; ++k) fact *= (double)k;  // (n - 1)!
  for (int i = 0; i < n; ++i) {
    double f, f1;
    hermite_e(n, prev[i], &f, &f1);
    w[i] = fact / ((double)n * f1 * f1);
    z[i] = prev[i];
  }
  for (int i = 0; i < n / 2; ++i) w[n - 1 - i] = w[i];
  for (int i = 0; i < n; ++i) sum += w[i];
  for (int i = 0; i < n; ++i) w[i] /= sum;
}
}  // namespace

int cilqr_pose_quadrature(int nx, int ny, int nth, double* nodes, double* weights) {
  if (!nodes || !weights) return fail(CILQR_ERR_ARG, "cilqr_pose_quadrature: null pointer");
  if (nx < 1 || nx > 9 || ny < 1 || ny > 9 || nth < 1 || nth > 9)
    return fail(CILQR_ERR_ARG, "cilqr_pose_quadrature: %d x %d x %d nodes, each axis takes 1 ... 9", nx, ny, nth);
  double zx[9], wx[9], zy[9], wy[9], zt[9], wt[9];
  gauss_hermite_e(nx, zx, wx);
  gauss_hermite_e(ny, zy, wy);
  gauss_hermite_e(nth, zt, wt);
  size_t q = 0;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nth; ++k, ++q) {
        nodes[3 * q] = zx[i]; nodes[3 * q + 1] = zy[j]; nodes[3 * q + 2] = zt[k];
        weights[q] = wx[i] * wy[j] * wt[k];
      }
  return CILQR_OK;
}

int cilqr_chance_risk_map_device(cilqr_handle* h, void* stream, int B, int N, int Q, const double* X, const double* sigma,
                                 const double* nodes, const double* weights, double occ_threshold, uint32_t flags, double max_risk,
                                 const double* base, double* risk, double* step_risk, double* step_occ, double* step_unknown,
                                 double* total) {
  int rc = chance_map_args_check(Q, X, sigma, nodes, weights, occ_threshold, flags, max_risk, base, risk, total);
  if (rc) return rc;
  rc = chance_map_handle_check(h, B, N);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::ChanceMapArgs a = {};
  a.s = handle_args(h, B, N, 0, 0);
  a.X = X; a.sigma = sigma; a.nodes = nodes; a.weights = weights;
  a.occ_threshold = occ_threshold; a.max_risk = max_risk; a.base = base; a.risk = risk; a.total = total;
  // a per-step output the caller did not ask for lives in the handle's own memory: the finish kernel reads all three
  const size_t slab = (size_t)h->max_batch * h->max_horizon;
  a.step_risk = step_risk ? step_risk : h->d_chance_map_steps;
  a.step_occ = step_occ ? step_occ : h->d_chance_map_steps + slab;
  a.step_unknown = step_unknown ? step_unknown : h->d_chance_map_steps + 2 * slab;
  a.partials = h->d_risk_part; a.part_stride = (long long)h->risk_part_stride;
  a.Q = Q; a.G = (N + cilqr::CHANCE_MAP_WAVES - 1) / cilqr::CHANCE_MAP_WAVES;
  a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_chance_risk_map(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_chance_risk_map(cilqr_handle* h, int B, int N, int Q, const double* X, const double* sigma, const double* nodes,
                          const double* weights, double occ_threshold, uint32_t flags, double max_risk, const double* base,
                          double* risk, double* step_risk, double* step_occ, double* step_unknown, double* total) {
  int rc = chance_map_args_check(Q, X, sigma, nodes, weights, occ_threshold, flags, max_risk, base, risk, total);
  if (rc) return rc;
  for (int q = 0; q < Q; ++q)
    if (!(weights[q] >= 0.0 && weights[q] <= 1.7e308))
      return fail(CILQR_ERR_ARG, "cilqr_chance_risk_map: weight %d is negative or not finite", q);
  rc = chance_map_handle_check(h, B, N);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_chance_risk_map(p, B, N, Q, X, sigma, nodes, weights, base, risk, step_risk, step_occ, step_unknown, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_chance_risk_map_device(h, h->stream, B, N, Q, X, sigma, nodes, weights, occ_threshold, flags, max_risk, base, risk,
                                        step_risk, step_occ, step_unknown, total);
  });
}

// ---- exact footprint check (cilqr_footprint.hip) ------------------------------------------------------------------------------------------
namespace {
// what needs no handle
int footprint_args_check(int M, int S, const double* X, const cilqr_obstacles* obs, double margin, double min_clearance,
                         double occ_threshold, uint32_t flags, const double* base, const double* fp, const double* total) {
  if (!X || !fp) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: null required pointer");
  if (M > 0 && (!obs || !obs->pose || !obs->dim)) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: M = %d but obs, its pose or its dim is null", M);
  if (total && !base) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: total needs base");
  if (S < 1) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: S = %d, must be at least 1", S);
  if (M > 0 && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0 || obs->weight_batch_stride < 0))
    return fail(CILQR_ERR_ARG, "cilqr_footprint_check: negative stride");
  if (!(margin >= 0.0 && margin <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: margin is negative or not finite");
  if (min_clearance != min_clearance || occ_threshold != occ_threshold)
    return fail(CILQR_ERR_ARG, "cilqr_footprint_check: min_clearance or occ_threshold is NaN");
  if (flags & ~(CILQR_FOOTPRINT_UNKNOWN_HITS | CILQR_FOOTPRINT_SKIP_MAP))
    return fail(CILQR_ERR_ARG, "cilqr_footprint_check: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
int footprint_handle_check(const cilqr_handle* h, int B, int N, int M, int S, const cilqr_obstacles* obs, double margin, uint32_t flags,
                           size_t* span) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (B < 0 || (int64_t)B * S > h->max_batch) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: B*S = %lld outside [0,%d]", (long long)B * S, h->max_batch);
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = check_obstacles(B, N, M, obs, span, nullptr);
  if (rc) return rc;
  if ((int64_t)M * N > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: M * N beyond 2^31 - 1 entries");
  if (h->unc.layer && !(flags & CILQR_FOOTPRINT_SKIP_MAP)) {
    if ((int64_t)h->unc.rows * h->unc.cols > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_footprint_check: the map has 2^31 cells or more");
    const double hl = 0.5 * h->params.length + margin, hw = 0.5 * h->params.width + margin;
    if (!(ceil(2.0 * hypot(hl, hw) / h->unc_res) + 2.0 <= 1024.0))
      return fail(CILQR_ERR_UNSUPPORTED, "cilqr_footprint_check: the footprint spans more than 1024 cells of %g m", h->unc_res);
  }
  return CILQR_OK;
}
}  // namespace

int cilqr_footprint_check_device(cilqr_handle* h, void* stream, int B, int N, int M, int S, const double* X, const cilqr_obstacles* obs,
                                 double margin, double min_clearance, double occ_threshold, uint32_t flags, const double* base,
                                 double* fp, double* step_clearance, float* step_occ, double* total) {
  int rc = footprint_args_check(M, S, X, obs, margin, min_clearance, occ_threshold, flags, base, fp, total);
  if (rc) return rc;
  rc = footprint_handle_check(h, B, N, M, S, obs, margin, flags, nullptr);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::FootprintArgs a = {};
  a.s = handle_args(h, B, N, M, 0);
  set_obstacles(a.s, M, obs);
  a.X = X;
  a.hl = 0.5 * h->params.length + margin; a.hw = 0.5 * h->params.width + margin;
  a.min_clearance = min_clearance; a.occ_threshold = occ_threshold; a.res = h->unc_res;
  a.base = base; a.fp = fp; a.step_occ = step_occ; a.total = total;
  a.rows = B * S; a.S = S; a.flags = flags;
  a.map_on = h->unc.layer && !(flags & CILQR_FOOTPRINT_SKIP_MAP) ? 1 : 0;
  // reserved at create: max_batch·max_horizon step records, max_batch row records, max_batch·max_horizon stand-in step clearances
  const size_t slab = (size_t)h->max_batch * h->max_horizon;
  a.steps = h->d_footprint_steps;
  a.row_rec = a.steps + slab * cilqr::FOOTPRINT_STEP_REC;
  a.step_clearance = step_clearance ? step_clearance : a.row_rec + (size_t)h->max_batch * cilqr::FOOTPRINT_ROW_REC;
  if ((int64_t)a.rows * ((N + cilqr::FOOTPRINT_WAVES - 1) / cilqr::FOOTPRINT_WAVES) > 0x7fffffff)
    return fail(CILQR_ERR_ARG, "cilqr_footprint_check: B * S * ceil(N / 4) workgroups beyond 2^31 - 1");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_footprint_check(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_footprint_check(cilqr_handle* h, int B, int N, int M, int S, const double* X, const cilqr_obstacles* obs, double margin,
                          double min_clearance, double occ_threshold, uint32_t flags, const double* base, double* fp,
                          double* step_clearance, float* step_occ, double* total) {
  int rc = footprint_args_check(M, S, X, obs, margin, min_clearance, occ_threshold, flags, base, fp, total);
  if (rc) return rc;
  size_t span = 0;
  rc = footprint_handle_check(h, B, N, M, S, obs, margin, flags, &span);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr_obstacles o = M > 0 ? *obs : cilqr_obstacles{};
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_footprint(p, (size_t)B * S, N, M, X, o, span, base, fp, step_clearance, step_occ, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_footprint_check_device(h, h->stream, B, N, M, S, X, &o, margin, min_clearance, occ_threshold, flags, base, fp,
                                        step_clearance, step_occ, total);
  });
}

// ---- distance to the occupied cells of a layer: exact field and inflation (costmap_distance.hip) -------------------------------------------
namespace {
// what needs no handle: L, the geometry and the stride of cilqr_map_distance and cilqr_inflate_map; *cells and *span (floats the
// layers' stride addresses) on success
int map_layers_check(const char* name, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, size_t* cells, size_t* span) {
  if (!layer || !g) return fail(CILQR_ERR_ARG, "%s: null layer or geometry", name);
  if (L < 1) return fail(CILQR_ERR_ARG, "%s: L = %d, must be at least 1", name, L);
  if (g->rows < 1 || g->cols < 1 || !(g->res > 0.0 && g->res <= 1.7e308)) return fail(CILQR_ERR_ARG, "%s: bad geometry", name);
  if (g->rows > cilqr::MAP_DISTANCE_MAX_SIDE || g->cols > cilqr::MAP_DISTANCE_MAX_SIDE)
    return fail(CILQR_ERR_UNSUPPORTED, "%s: %d x %d cells, more than %d along a side", name, g->rows, g->cols, cilqr::MAP_DISTANCE_MAX_SIDE);
  const int64_t n = (int64_t)g->rows * g->cols;
  if (layer_stride < 0 || (layer_stride > 0 && layer_stride < n)) return fail(CILQR_ERR_ARG, "%s: layer_stride smaller than one layer", name);
  if (layer_stride > ((int64_t)1 << 40)) return fail(CILQR_ERR_ARG, "%s: layer_stride beyond 2^40", name);
  const int64_t tiles = (n + cilqr::MAP_DISTANCE_THREADS - 1) / cilqr::MAP_DISTANCE_THREADS;
  if ((int64_t)L * (tiles > g->cols ? tiles : g->cols) > 0x7fffffff) return fail(CILQR_ERR_ARG, "%s: L = %d layers beyond 2^31 - 1 workgroups", name, L);
  *cells = (size_t)n;
  *span = (size_t)((int64_t)(L - 1) * layer_stride + n);
  return CILQR_OK;
}
int map_distance_args_check(int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, double occ_threshold, uint32_t flags,
                            const int32_t* d2_out, size_t* cells, size_t* span) {
  if (!d2_out) return fail(CILQR_ERR_ARG, "cilqr_map_distance: null d2_out");
  int rc = map_layers_check("cilqr_map_distance", L, layer, layer_stride, g, cells, span);
  if (rc) return rc;
  if (occ_threshold != occ_threshold) return fail(CILQR_ERR_ARG, "cilqr_map_distance: occ_threshold is NaN");
  if (flags & ~(CILQR_MAP_DISTANCE_UNKNOWN_SEEDS | CILQR_MAP_DISTANCE_TO_FREE)) return fail(CILQR_ERR_ARG, "cilqr_map_distance: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
int inflate_map_args_check(int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, const int32_t* d2, double inscribed,
                           double radius, double peak, const float* layer_out, size_t* cells, size_t* span) {
  if (!d2 || !layer_out) return fail(CILQR_ERR_ARG, "cilqr_inflate_map: null d2 or layer_out");
  int rc = map_layers_check("cilqr_inflate_map", L, layer, layer_stride, g, cells, span);
  if (rc) return rc;
  if (!(inscribed >= 0.0 && radius <= 1.7e308 && inscribed < radius)) return fail(CILQR_ERR_ARG, "cilqr_inflate_map: needs 0 <= inscribed < radius, both finite");
  if (!(peak > 0.0 && peak <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_inflate_map: peak is not finite and > 0");
  return CILQR_OK;
}
}  // namespace

int cilqr_map_distance_device(cilqr_handle* h, void* stream, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g,
                              double occ_threshold, uint32_t flags, int32_t* d2_out, float* dist_out) {
  size_t cells = 0, span = 0;
  int rc = map_distance_args_check(L, layer, layer_stride, g, occ_threshold, flags, d2_out, &cells, &span);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::MapDistanceArgs a = {};
  a.layer = layer; a.layer_stride = layer_stride; a.d2_out = d2_out; a.dist_out = dist_out;
  a.occ_threshold = occ_threshold; a.res = g->res;
  a.L = L; a.rows = g->rows; a.cols = g->cols; a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_map_distance(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_map_distance(cilqr_handle* h, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, double occ_threshold,
                       uint32_t flags, int32_t* d2_out, float* dist_out) {
  size_t cells = 0, span = 0;
  int rc = map_distance_args_check(L, layer, layer_stride, g, occ_threshold, flags, d2_out, &cells, &span);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_map_distance(p, L, cells, span, layer, d2_out, dist_out);
  return cilqr::host_call(h, p, [&] { return cilqr_map_distance_device(h, h->stream, L, layer, layer_stride, g, occ_threshold, flags, d2_out, dist_out); });
}

int cilqr_inflate_map_device(cilqr_handle* h, void* stream, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g,
                             const int32_t* d2, double inscribed, double radius, double peak, float* layer_out) {
  size_t cells = 0, span = 0;
  int rc = inflate_map_args_check(L, layer, layer_stride, g, d2, inscribed, radius, peak, layer_out, &cells, &span);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  // lane = cell reads its own cell and writes it: in place is fine where layer l of the output IS layer l of the input
  const bool same = layer_out == layer && (L == 1 || (size_t)layer_stride == cells);
  if (!same && layer_out < layer + span && layer < layer_out + (size_t)L * cells)
    return fail(CILQR_ERR_ARG, "cilqr_inflate_map: layer_out overlaps layer without being the same layers");
  cilqr::InflateMapArgs a = {};
  a.layer = layer; a.layer_stride = layer_stride; a.d2 = d2; a.layer_out = layer_out;
  a.res = g->res; a.inscribed = inscribed; a.radius = radius; a.peak = peak;
  a.L = L; a.rows = g->rows; a.cols = g->cols;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_inflate_map(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_inflate_map(cilqr_handle* h, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, const int32_t* d2,
                      double inscribed, double radius, double peak, float* layer_out) {
  size_t cells = 0, span = 0;
  int rc = inflate_map_args_check(L, layer, layer_stride, g, d2, inscribed, radius, peak, layer_out, &cells, &span);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_inflate_map(p, L, cells, span, layer, d2, layer_out);
  return cilqr::host_call(h, p, [&] { return cilqr_inflate_map_device(h, h->stream, L, layer, layer_stride, g, d2, inscribed, radius, peak, layer_out); });
}

// ---- obstacles from the map: connected components of occupied cells as boxes (costmap_components.hip) ---------------------------------------
namespace {
// what needs no handle; *cells on success
int map_obstacles_args_check(int L, const int32_t* d2, const cilqr_map_geom* g, int gap2, uint32_t flags, int pose_stride, int K,
                             int min_cells, double max_size, double pad, const int32_t* work, const int32_t* label_out,
                             const int32_t* n_out, const double* comp, size_t* cells) {
  if (!d2 || !g || !work || !label_out || !n_out || !comp) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: null required pointer");
  if (g->rows > cilqr::MAP_OBSTACLES_MAX_SIDE || g->cols > cilqr::MAP_OBSTACLES_MAX_SIDE)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_map_obstacles: %d x %d cells, more than %d along a side", g->rows, g->cols,
                cilqr::MAP_OBSTACLES_MAX_SIDE);
  size_t span = 0;
  // (the geometry and L as cilqr_map_distance takes them: d2 stands in for its layers, dense)
  int rc = map_layers_check("cilqr_map_obstacles", L, (const float*)d2, 0, g, cells, &span);
  if (rc) return rc;
  if (gap2 < 0) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: gap2 = %d is negative", gap2);
  if (flags & ~CILQR_MAP_OBSTACLES_FOUR) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: unknown flag bits 0x%x", flags);
  if (pose_stride != 0 && pose_stride != 3) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: pose_stride = %d, must be 0 or 3", pose_stride);
  if (K < 1 || K > CILQR_MAX_POLYGONS) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: K = %d outside [1,%d]", K, CILQR_MAX_POLYGONS);
  if (min_cells < 1) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: min_cells = %d, must be at least 1", min_cells);
  if (!(max_size > 0.0)) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: max_size is not > 0");
  if (!(pad >= 0.0 && pad <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: pad is negative or not finite");
  const int64_t tiles = (int64_t)((g->rows + cilqr::CC_TILE_I - 1) / cilqr::CC_TILE_I) * ((g->cols + cilqr::CC_TILE_J - 1) / cilqr::CC_TILE_J);
  if ((int64_t)L * (tiles > K ? tiles : K) > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_map_obstacles: L = %d layers beyond 2^31 - 1 workgroups", L);
  return CILQR_OK;
}
}  // namespace

int cilqr_map_obstacles_device(cilqr_handle* h, void* stream, int L, const int32_t* d2, const cilqr_map_geom* g, int gap2, uint32_t flags,
                               const double* pose, int pose_stride, int K, int min_cells, double max_size, double pad, int32_t* work,
                               int32_t* label_out, int32_t* n_out, double* comp, double* boxes, double* pose_out, double* dim_out) {
  size_t cells = 0;
  int rc = map_obstacles_args_check(L, d2, g, gap2, flags, pose_stride, K, min_cells, max_size, pad, work, label_out, n_out, comp, &cells);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::MapObstaclesArgs a = {};
  a.d2 = d2; a.pose = pose; a.work = work; a.label_out = label_out; a.n_out = n_out; a.comp = comp;
  a.boxes = boxes; a.pose_out = pose_out; a.dim_out = dim_out;
  a.res = g->res;
  a.x_first = g->pos_x + (0.5 * g->len_x - 0.5 * g->res);  // cell (0,0) centre, as the uncertainty map forms it
  a.y_first = g->pos_y + (0.5 * g->len_y - 0.5 * g->res);
  a.max_size = max_size; a.pad = pad;
  a.L = L; a.rows = g->rows; a.cols = g->cols; a.gap2 = gap2; a.K = K; a.min_cells = min_cells; a.pose_stride = pose_stride;
  a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_map_obstacles(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_map_obstacles(cilqr_handle* h, int L, const int32_t* d2, const cilqr_map_geom* g, int gap2, uint32_t flags, const double* pose,
                        int pose_stride, int K, int min_cells, double max_size, double pad, int32_t* work, int32_t* label_out,
                        int32_t* n_out, double* comp, double* boxes, double* pose_out, double* dim_out) {
  size_t cells = 0;
  int rc = map_obstacles_args_check(L, d2, g, gap2, flags, pose_stride, K, min_cells, max_size, pad, work, label_out, n_out, comp, &cells);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  const int32_t* counts = n_out;  // the caller's, read once the results are back
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_map_obstacles(p, L, cells, K, pose ? (pose_stride ? L : 1) : 0, d2, pose, work, label_out, n_out, comp, boxes, pose_out, dim_out);
  rc = cilqr::host_call(h, p, [&] {
    return cilqr_map_obstacles_device(h, h->stream, L, d2, g, gap2, flags, pose, pose_stride, K, min_cells, max_size, pad, work, label_out,
                                      n_out, comp, boxes, pose_out, dim_out);
  });
  if (rc) return rc;
  for (int l = 0; l < L; ++l)
    if (counts[4 * l + 2] < 0) return fail(CILQR_ERR_INTERNAL, "cilqr_map_obstacles: a loop bound ran out in layer %d", l);
  return CILQR_OK;
}

// ---- static layer: the cells of tracked movers taken out of the map (costmap_movers.hip) -----------------------------------------------------
namespace {
// what needs no handle; *cells, *span and *tracker (which mover form) on success
int clear_movers_args_check(int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, const int32_t* label, int K,
                            const double* comp, int M, const int32_t* assign, const double* state, int min_hits, double v_clear,
                            const int32_t* mask, int halo2, float fill, const float* layer_out, const double* fields, size_t* cells,
                            size_t* span, bool* tracker) {
  if (!layer || !g || !label || !comp || !layer_out || !fields) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: null required pointer");
  if (g->rows > cilqr::MAP_OBSTACLES_MAX_SIDE || g->cols > cilqr::MAP_OBSTACLES_MAX_SIDE)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_clear_movers: %d x %d cells, more than %d along a side", g->rows, g->cols,
                cilqr::MAP_OBSTACLES_MAX_SIDE);
  int rc = map_layers_check("cilqr_clear_movers", L, layer, layer_stride, g, cells, span);
  if (rc) return rc;
  if (K < 1 || K > CILQR_MAX_POLYGONS) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: K = %d outside [1,%d]", K, CILQR_MAX_POLYGONS);
  const bool by_tracker = assign && state && !mask, by_mask = mask && !assign && !state;
  if (!by_tracker && !by_mask)
    return fail(CILQR_ERR_ARG, "cilqr_clear_movers: the movers come as assign and state, or as mask: exactly one of the two forms");
  if (by_tracker) {
    if (M < 1 || M > CILQR_TRACK_MAX_SLOTS) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: M = %d outside [1,%d]", M, CILQR_TRACK_MAX_SLOTS);
    if (min_hits < 1) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: min_hits = %d, must be at least 1", min_hits);
    if (!(v_clear >= 0.0)) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: v_clear is negative or NaN");
  }
  if (halo2 < 0 || halo2 > CILQR_CLEAR_MOVERS_MAX_HALO2)
    return fail(CILQR_ERR_ARG, "cilqr_clear_movers: halo2 = %d outside [0,%d]", halo2, CILQR_CLEAR_MOVERS_MAX_HALO2);
  if (fill == fill && fill - fill != 0.0f) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: fill is infinite");
  const int64_t tiles = (int64_t)((g->rows + cilqr::CM_TILE_I - 1) / cilqr::CM_TILE_I) * ((g->cols + cilqr::CM_TILE_J - 1) / cilqr::CM_TILE_J);
  if ((int64_t)L * tiles > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_clear_movers: L = %d layers beyond 2^31 - 1 workgroups", L);
  *tracker = by_tracker;
  return CILQR_OK;
}
}  // namespace

int cilqr_clear_movers_device(cilqr_handle* h, void* stream, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g,
                              const int32_t* label, int K, const double* comp, int M, const int32_t* assign, const double* state,
                              int min_hits, double v_clear, const int32_t* mask, int halo2, float fill, float* layer_out,
                              int32_t* owner_out, double* fields) {
  size_t cells = 0, span = 0;
  bool tracker = false;
  int rc = clear_movers_args_check(L, layer, layer_stride, g, label, K, comp, M, assign, state, min_hits, v_clear, mask, halo2, fill,
                                   layer_out, fields, &cells, &span, &tracker);
  if (rc) return rc;
  // lane = cell reads its own cell and writes it: in place is fine where layer l of the output IS layer l of the input
  const bool same = layer_out == layer && (L == 1 || (size_t)layer_stride == cells);
  if (!same && layer_out < layer + span && layer < layer_out + (size_t)L * cells)
    return fail(CILQR_ERR_ARG, "cilqr_clear_movers: layer_out overlaps layer without being the same layers");
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::ClearMoversArgs a = {};
  a.layer = layer; a.layer_stride = layer_stride; a.label = label; a.comp = comp;
  a.assign = tracker ? assign : nullptr; a.state = tracker ? state : nullptr; a.mask = tracker ? nullptr : mask;
  a.layer_out = layer_out; a.owner_out = owner_out; a.fields = fields;
  a.v_clear = v_clear; a.fill = fill;
  a.L = L; a.rows = g->rows; a.cols = g->cols; a.K = K; a.M = tracker ? M : 0; a.min_hits = min_hits; a.halo2 = halo2;
  a.r = cilqr::cm_isqrt(halo2);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_clear_movers(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_clear_movers(cilqr_handle* h, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, const int32_t* label,
                       int K, const double* comp, int M, const int32_t* assign, const double* state, int min_hits, double v_clear,
                       const int32_t* mask, int halo2, float fill, float* layer_out, int32_t* owner_out, double* fields) {
  size_t cells = 0, span = 0;
  bool tracker = false;
  int rc = clear_movers_args_check(L, layer, layer_stride, g, label, K, comp, M, assign, state, min_hits, v_clear, mask, halo2, fill,
                                   layer_out, fields, &cells, &span, &tracker);
  if (rc) return rc;
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  cilqr::HostPlan p(h->d_arena);
  // (in the arena the output has a place of its own, whatever the caller's two host addresses are)
  cilqr::plan_clear_movers(p, L, cells, span, K, tracker ? M : 0, layer, label, comp, assign, state, mask, layer_out, owner_out, fields);
  return cilqr::host_call(h, p, [&] {
    return cilqr_clear_movers_device(h, h->stream, L, layer, layer_stride, g, label, K, comp, M, assign, state, min_hits, v_clear, mask,
                                     halo2, fill, layer_out, owner_out, fields);
  });
}

// ---- exact clearance of the ego rectangle to the occupied cells of the map (cilqr_map_clearance.hip) ---------------------------------------
namespace {
// what needs no handle
int map_clearance_args_check(int S, const double* X, double margin, double occ_threshold, double reach, double min_clearance, uint32_t flags,
                             const double* base, const double* mc, const double* total) {
  if (!X || !mc) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: null required pointer");
  if (total && !base) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: total needs base");
  if (S < 1) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: S = %d, must be at least 1", S);
  if (!(margin >= 0.0 && margin <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: margin is negative or not finite");
  if (!(reach >= 0.0 && reach <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: reach is negative or not finite");
  if (min_clearance != min_clearance || occ_threshold != occ_threshold)
    return fail(CILQR_ERR_ARG, "cilqr_map_clearance: min_clearance or occ_threshold is NaN");
  if (flags & ~CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
int map_clearance_handle_check(const cilqr_handle* h, int B, int N, int S, double margin, double reach) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (B < 0 || (int64_t)B * S > h->max_batch) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: B*S = %lld outside [0,%d]", (long long)B * S, h->max_batch);
  int rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  if (!h->unc.layer) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: no uncertainty map is set on the handle");
  if ((int64_t)h->unc.rows * h->unc.cols > 0x7fffffff) return fail(CILQR_ERR_ARG, "cilqr_map_clearance: the map has 2^31 cells or more");
  const double hl = 0.5 * h->params.length + margin, hw = 0.5 * h->params.width + margin;
  if (!(ceil(2.0 * (hypot(hl, hw) + reach) / h->unc_res) + 2.0 <= 1024.0))
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_map_clearance: the search window spans more than 1024 cells of %g m", h->unc_res);
  return CILQR_OK;
}
}  // namespace

int cilqr_map_clearance_device(cilqr_handle* h, void* stream, int B, int N, int S, const double* X, double margin, double occ_threshold,
                               double reach, double min_clearance, uint32_t flags, const double* base, double* mc,
                               double* step_clearance, double* total) {
  int rc = map_clearance_args_check(S, X, margin, occ_threshold, reach, min_clearance, flags, base, mc, total);
  if (rc) return rc;
  rc = map_clearance_handle_check(h, B, N, S, margin, reach);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::MapClearanceArgs a = {};
  a.s = handle_args(h, B, N, 0, 0);
  a.X = X;
  a.hl = 0.5 * h->params.length + margin; a.hw = 0.5 * h->params.width + margin;
  a.reach = reach; a.min_clearance = min_clearance; a.occ_threshold = occ_threshold; a.res = h->unc_res;
  a.base = base; a.mc = mc; a.total = total;
  a.rows = B * S; a.S = S; a.flags = flags;
  // the footprint check's region, reserved at create: max_batch·max_horizon step records, then stand-in step clearances
  const size_t slab = (size_t)h->max_batch * h->max_horizon;
  a.steps = h->d_footprint_steps;
  a.step_clearance = step_clearance ? step_clearance : a.steps + slab * cilqr::MAP_CLEARANCE_STEP_REC;
  if ((int64_t)a.rows * ((N + cilqr::FOOTPRINT_WAVES - 1) / cilqr::FOOTPRINT_WAVES) > 0x7fffffff)
    return fail(CILQR_ERR_ARG, "cilqr_map_clearance: B * S * ceil(N / 4) workgroups beyond 2^31 - 1");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_map_clearance(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_map_clearance(cilqr_handle* h, int B, int N, int S, const double* X, double margin, double occ_threshold, double reach,
                        double min_clearance, uint32_t flags, const double* base, double* mc, double* step_clearance, double* total) {
  int rc = map_clearance_args_check(S, X, margin, occ_threshold, reach, min_clearance, flags, base, mc, total);
  if (rc) return rc;
  rc = map_clearance_handle_check(h, B, N, S, margin, reach);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_map_clearance(p, (size_t)B * S, N, X, base, mc, step_clearance, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_map_clearance_device(h, h->stream, B, N, S, X, margin, occ_threshold, reach, min_clearance, flags, base, mc, step_clearance, total);
  });
}

// ---- stop plans: a solved plan's geometry under a braking profile (cilqr_stop.hip) ------------------------------------------------------
namespace {
// what needs no handle
int stop_args_check(int D, const double* X, const double* U, const double* decel, int hold, double max_deviation, double decel_weight,
                    uint32_t flags, const double* X_stop, const double* U_stop, const double* sp) {
  if (!X || !U || !decel || !X_stop || !U_stop || !sp) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: null required pointer");
  if (D < 1) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: D = %d, must be at least 1", D);
  if (hold < 0) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: hold = %d is negative", hold);
  if (!(max_deviation >= 0.0)) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: max_deviation is negative or NaN");
  if (!(fabs(decel_weight) <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: decel_weight is not finite");
  if (flags & ~CILQR_STOP_ALLOW_MOVING) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
// the levels of the host-buffer form, which it can read
int stop_levels_check(int D, const double* decel) {
  for (int l = 0; l < D; ++l)
    if (!(decel[l] > 0.0 && decel[l] <= 1.7e308)) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: decel[%d] is not finite or not positive", l);
  return CILQR_OK;
}
int stop_handle_check(const cilqr_handle* h, int B, int N, int D) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (B < 0 || (int64_t)B * D > h->max_batch) return fail(CILQR_ERR_ARG, "cilqr_stop_plans: B*D = %lld outside [0,%d]", (long long)B * D, h->max_batch);
  int rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  return CILQR_OK;  // (every horizon a handle accepts fits the kernel's LDS: a static_assert in cilqr_stop.hip)
}
}  // namespace

int cilqr_stop_plans_device(cilqr_handle* h, void* stream, int B, int N, int D, const double* X, const double* U, const double* decel,
                            int hold, double max_deviation, const double* plan_cost, double decel_weight, uint32_t flags,
                            double* X_stop, double* U_stop, double* sp, double* cost) {
  int rc = stop_args_check(D, X, U, decel, hold, max_deviation, decel_weight, flags, X_stop, U_stop, sp);
  if (rc) return rc;
  rc = stop_handle_check(h, B, N, D);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::StopArgs a = {};
  a.X = X; a.U = U; a.decel = decel; a.plan_cost = plan_cost;
  a.X_stop = X_stop; a.U_stop = U_stop; a.sp = sp; a.cost = cost;
  a.max_deviation = max_deviation; a.decel_weight = decel_weight;
  a.B = B; a.N = N; a.D = D; a.hold = hold; a.flags = flags;
  a.plans = cilqr::stop_plans_per_group(N, D);
  a.dt = h->kp.dt; a.half_dt2 = h->kp.half_dt2; a.acc_max = h->kp.acc_max; a.acc_min = h->kp.acc_min;
  a.yaw_hi = h->kp.yaw_hi; a.yaw_lo = h->kp.yaw_lo; a.speed_max = h->kp.speed_max;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_stop_plans(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_stop_plans(cilqr_handle* h, int B, int N, int D, const double* X, const double* U, const double* decel, int hold,
                     double max_deviation, const double* plan_cost, double decel_weight, uint32_t flags, double* X_stop, double* U_stop,
                     double* sp, double* cost) {
  int rc = stop_args_check(D, X, U, decel, hold, max_deviation, decel_weight, flags, X_stop, U_stop, sp);
  if (rc) return rc;
  rc = stop_levels_check(D, decel);
  if (rc) return rc;
  rc = stop_handle_check(h, B, N, D);
  if (rc) return rc;
  for (int l = 0; l < D; ++l)
    if (decel[l] > -h->params.acc_min)
      return fail(CILQR_ERR_ARG, "cilqr_stop_plans: decel[%d] = %g is above -acc_min = %g, the model would clamp it", l, decel[l], -h->params.acc_min);
  if (B == 0) return CILQR_OK;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_stop_plans(p, B, N, D, X, U, decel, plan_cost, X_stop, U_stop, sp, cost);
  return cilqr::host_call(h, p, [&] {
    return cilqr_stop_plans_device(h, h->stream, B, N, D, X, U, decel, hold, max_deviation, plan_cost, decel_weight, flags, X_stop, U_stop, sp, cost);
  });
}

// ---- analytic chance risk against sampled obstacles in compact form (cilqr_chance_sampled.hip) ----------------------------------------
namespace {
// what needs no handle
int chance_sampled_args_check(int n_obs, int n_samples, const double* X, const double* sigma, const double* nom_pose, const double* nom_dim,
                              const double* sample_offset, uint32_t flags, double max_risk, const double* base, const double* risk,
                              const double* total) {
  if (!X || !sigma || !nom_pose || !nom_dim || !sample_offset || !risk)
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: null required pointer");
  if (total && !base) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: total needs base");
  if (n_obs < 1 || n_samples < 2) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: needs n_obs >= 1 and n_samples >= 2");
  if (max_risk != max_risk) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: max_risk is NaN");
  if (flags & ~CILQR_CHANCE_SAMPLED_BOUND_SUM) return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: unknown flag bits 0x%x", flags);
  return CILQR_OK;
}
int chance_sampled_handle_check(const cilqr_handle* h, int B, int N, int n_obs, int n_samples) {
  int rc = check_sampled(h, "cilqr_chance_risk_sampled", B, N, n_obs, n_samples);
  if (rc) return rc;
  // every index the kernels keep in 32 bits: an entry m*N + t, the grid
  if ((int64_t)n_obs * n_samples * N > 0x7fffffff)
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: n_obs * n_samples * N beyond 2^31 entries");
  const int64_t G = ((int64_t)N + cilqr::CHANCE_SAMPLED_WAVES - 1) / cilqr::CHANCE_SAMPLED_WAVES;
  if ((int64_t)B * G > 0x7fffffff)
    return fail(CILQR_ERR_ARG, "cilqr_chance_risk_sampled: B * ceil(N/%d) beyond 2^31 workgroups", cilqr::CHANCE_SAMPLED_WAVES);
  return CILQR_OK;
}
}  // namespace

int cilqr_chance_risk_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* X,
                                     const double* sigma, const double* nom_pose, const double* nom_dim, const double* sample_offset,
                                     uint32_t flags, double max_risk, const double* base, double* risk, double* step_risk,
                                     double* pair_p, double* entry_p, double* total) {
  int rc = chance_sampled_args_check(n_obs, n_samples, X, sigma, nom_pose, nom_dim, sample_offset, flags, max_risk, base, risk, total);
  if (rc) return rc;
  rc = chance_sampled_handle_check(h, B, N, n_obs, n_samples);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  if (cilqr::chance_risk_sampled_lds_bytes(n_obs, n_samples) > cilqr::CHANCE_SAMPLED_LDS_MAX)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_chance_risk_sampled: %d x %d obstacle samples do not fit 64 KiB of LDS", n_obs, n_samples);
  cilqr::ChanceSampledArgs a = {};
  a.s = handle_args(h, B, N, n_obs, 0);
  a.s.obs_pose = nom_pose; a.s.obs_dim = nom_dim;
  a.s.samp_off = sample_offset; a.s.n_samples = n_samples;
  a.X = X; a.sigma = sigma;
  a.max_risk = max_risk; a.base = base; a.risk = risk; a.step_risk = step_risk; a.pair_p = pair_p; a.entry_p = entry_p; a.total = total;
  a.steps = h->d_chance_sampled_steps;
  a.G = (N + cilqr::CHANCE_SAMPLED_WAVES - 1) / cilqr::CHANCE_SAMPLED_WAVES;
  a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_chance_risk_sampled(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_chance_risk_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* sigma,
                              const double* nom_pose, const double* nom_dim, const double* sample_offset, uint32_t flags,
                              double max_risk, const double* base, double* risk, double* step_risk, double* pair_p, double* entry_p,
                              double* total) {
  int rc = chance_sampled_args_check(n_obs, n_samples, X, sigma, nom_pose, nom_dim, sample_offset, flags, max_risk, base, risk, total);
  if (rc) return rc;
  rc = chance_sampled_handle_check(h, B, N, n_obs, n_samples);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::HostPlan p(h->d_arena);
  cilqr::plan_chance_sampled(p, B, N, n_obs, n_samples, X, sigma, nom_pose, nom_dim, sample_offset, base, risk, step_risk, pair_p,
                             entry_p, total);
  return cilqr::host_call(h, p, [&] {
    return cilqr_chance_risk_sampled_device(h, h->stream, B, N, n_obs, n_samples, X, sigma, nom_pose, nom_dim, sample_offset, flags,
                                            max_risk, base, risk, step_risk, pair_p, entry_p, total);
  });
}

// kappa with erfc(kappa/sqrt 2)/2 = eps: Newton's iteration on log erfc, whose graph is nearly a parabola, from
// sqrt(-2 log eps) — at or beyond the root, since erfc(k/sqrt 2)/2 <= exp(-k^2/2)/2 — with a fixed number of steps.
double cilqr_chance_kappa(double eps) {
  if (!(eps > 0.0 && eps <= 0.5)) return NAN;
  if (eps == 0.5) return 0.0;
  const double root_half = 7.07106781186547524401e-01, inv_root_2pi = 3.98942280401432677940e-01;
  double k = sqrt(-2.0 * log(eps));
  for (int i = 0; i < 40; ++i) {
    const double q = 0.5 * erfc(k * root_half);
    if (!(q > 0.0)) { k -= 0.5; continue; }  // (underflow, eps below 1e-300: back towards the root)
    k += q / (inv_root_2pi * exp(-0.5 * k * k)) * log(q / eps);
  }
  return k;
}

int cilqr_blur_costmap_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* g, int index, double vtheta,
                              double sigma_x, double sigma_y, double sigma_theta, float* out, int32_t* count_out) {
  if (!h || !src || !g || !out) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap: null argument");
  if (g->rows < 1 || g->cols < 1 || !(g->res > 0.0) || index < 0) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap: bad geometry");
  HIP_TRY(hipSetDevice(h->device));
  cilqr::BlurArgs a;
  a.src = src; a.out = out; a.count_out = count_out;
  a.occ_out = nullptr; a.occ_min = 0.0f; a.occ_den = 100.0f;
  a.g = *g; a.index = index;
  a.sin_t = sin(vtheta);  // host libm, as the caller of the reference does (M/src/local_costmap.cpp:201-202)
  a.cos_t = cos(vtheta);
  a.sigma_x = sigma_x; a.sigma_y = sigma_y; a.sigma_theta = sigma_theta;
  HIP_TRY(cilqr::launch_blur(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_blur_costmap(cilqr_handle* h, const float* src, const cilqr_map_geom* g, int index, double vtheta, double sigma_x,
                       double sigma_y, double sigma_theta, float* out, int32_t* count_out) {
  if (!h || !src || !g || !out) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap: null argument");
  if (g->rows < 1 || g->cols < 1) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap: bad geometry");
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)g->rows * g->cols;
  int rc = grow(&h->d_src, &h->src_cap, n);
  if (rc == CILQR_OK) rc = grow(&h->d_dst, &h->dst_cap, n);
  if (rc) return rc;
  void* v_cnt = nullptr;
  if (count_out) {
    int rcs = cilqr::scratch_bytes(h, cilqr::SCR_COUNT, n * sizeof(int32_t), &v_cnt);
    if (rcs) return rcs;
  }
  int32_t* d_cnt = (int32_t*)v_cnt;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(h->d_src, src, n * sizeof(float), hipMemcpyHostToDevice, s));
  rc = cilqr_blur_costmap_device(h, s, h->d_src, g, index, vtheta, sigma_x, sigma_y, sigma_theta, h->d_dst, d_cnt);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, h->d_dst, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (count_out) HIP_TRY(hipMemcpyAsync(count_out, d_cnt, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CILQR_OK;
}

int cilqr_local_plan_batch_device(cilqr_handle* h, void* stream, int B, int P, const double* path, int64_t path_stride,
                                  const double* ego, double* poly, double* xplan_fl, double* ref_traj, int32_t* n_out) {
  if (!h || !path || !ego || !poly || !xplan_fl) return fail(CILQR_ERR_ARG, "cilqr_local_plan_batch: null argument");
  if (B < 1 || P < 1 || path_stride < 0) return fail(CILQR_ERR_ARG, "cilqr_local_plan_batch: bad size");
  const cilqr_params& p = h->params;
  if (p.num_of_local_wpts < 1 || p.poly_order < 0 || p.poly_order + 1 > CILQR_POLY_COEFFS)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_local_plan_batch: poly_order must be in [0, 5]");
  if (cilqr::local_plan_lds_bytes(p.num_of_local_wpts, p.poly_order + 1) > 64 * 1024)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_local_plan_batch: num_of_local_wpts too large for the per-candidate LDS slot");
  HIP_TRY(hipSetDevice(h->device));
  cilqr::LocalPlanArgs a;
  a.path = path; a.path_stride = path_stride; a.ego = ego;
  a.poly = poly; a.xplan_fl = xplan_fl; a.ref_traj = ref_traj; a.n_out = n_out;
  a.B = B; a.P = P; a.n_wpts = p.num_of_local_wpts; a.cols = p.poly_order + 1;
  HIP_TRY(cilqr::launch_local_plan(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_local_plan_batch(cilqr_handle* h, int B, int P, const double* path, int64_t path_stride, const double* ego,
                           double* poly, double* xplan_fl, double* ref_traj, int32_t* n_out) {
  if (!h || !path || !ego || !poly || !xplan_fl) return fail(CILQR_ERR_ARG, "cilqr_local_plan_batch: null argument");
  if (B < 1 || P < 1 || path_stride < 0) return fail(CILQR_ERR_ARG, "cilqr_local_plan_batch: bad size");
  HIP_TRY(hipSetDevice(h->device));
  const size_t W = h->params.num_of_local_wpts, b = B;
  const size_t n_path = path_stride ? (size_t)(B - 1) * path_stride + 2 * (size_t)P : 2 * (size_t)P;
  // device scratch owned by the handle (reserved at create for max_batch candidates; the path block grows with the first long path)
  void *vp = nullptr, *vio = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_PLAN_PATH, n_path * sizeof(double), &vp);
  if (rc) return rc;
  const size_t o_ego = 0, o_poly = o_ego + b * 4, o_fl = o_poly + b * CILQR_POLY_COEFFS, o_ref = o_fl + b * 2, o_n = o_ref + b * 2 * W;
  rc = cilqr::scratch_bytes(h, cilqr::SCR_PLAN_IO, o_n * sizeof(double) + b * sizeof(int32_t), &vio);
  if (rc) return rc;
  double* d_path = (double*)vp;
  double* io = (double*)vio;
  int32_t* d_n = (int32_t*)(io + o_n);
  hipStream_t s = h->stream;
  if (ref_traj) HIP_TRY(hipMemsetAsync(io + o_ref, 0, b * 2 * W * sizeof(double), s));
  HIP_TRY(hipMemcpyAsync(d_path, path, n_path * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(io + o_ego, ego, b * 4 * sizeof(double), hipMemcpyHostToDevice, s));
  rc = cilqr_local_plan_batch_device(h, s, B, P, d_path, path_stride, io + o_ego, io + o_poly, io + o_fl, ref_traj ? io + o_ref : nullptr,
                                     n_out ? d_n : nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(poly, io + o_poly, b * CILQR_POLY_COEFFS * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(xplan_fl, io + o_fl, b * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (ref_traj) HIP_TRY(hipMemcpyAsync(ref_traj, io + o_ref, b * 2 * W * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_out) HIP_TRY(hipMemcpyAsync(n_out, d_n, b * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CILQR_OK;
}

// ---- path-aligned planning frame (local_plan.hip, cilqr_frame.hip) ---------------------------------------------------------------------
namespace {
int local_plan_frames_check(const cilqr_handle* h, int B, int P, const double* path, int64_t path_stride, const double* ego,
                            const double* frames, const int32_t* info, const double* ego_out, const double* poly, const double* xplan_fl) {
  if (!h) return fail(CILQR_ERR_ARG, "null handle");
  if (!path || !ego || !frames || !info || !ego_out || !poly || !xplan_fl)
    return fail(CILQR_ERR_ARG, "cilqr_local_plan_frames: null required pointer");
  if (ego_out == ego) return fail(CILQR_ERR_ARG, "cilqr_local_plan_frames: ego_out must not be ego");
  if (B < 1 || B > h->max_batch) return fail(CILQR_ERR_ARG, "cilqr_local_plan_frames: B=%d outside [1,%d]", B, h->max_batch);
  if (P < 1) return fail(CILQR_ERR_ARG, "cilqr_local_plan_frames: P=%d must be at least 1", P);
  if (path_stride < 0) return fail(CILQR_ERR_ARG, "cilqr_local_plan_frames: negative path_stride");
  const cilqr_params& p = h->params;
  if (p.num_of_local_wpts < 1 || p.poly_order < 0 || p.poly_order + 1 > CILQR_POLY_COEFFS)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_local_plan_frames: poly_order must be in [0, 5]");
  if (cilqr::local_plan_lds_bytes(p.num_of_local_wpts, p.poly_order + 1) > 64 * 1024)
    return fail(CILQR_ERR_UNSUPPORTED, "cilqr_local_plan_frames: num_of_local_wpts too large for the per-candidate LDS slot");
  return CILQR_OK;
}

// frame_stride of the three transforms: `name` is the call's
int frame_stride_check(const char* name, const double* frames, int64_t frame_stride) {
  if (!frames) return fail(CILQR_ERR_ARG, "%s: frames is null", name);
  if (frame_stride != 0 && frame_stride != CILQR_FRAME_DOUBLES)
    return fail(CILQR_ERR_ARG, "%s: frame_stride=%lld is neither 0 nor %d", name, (long long)frame_stride, CILQR_FRAME_DOUBLES);
  return CILQR_OK;
}

int frame_obstacles_check(const cilqr_handle* h, int B, int N, int M, const double* frames, int64_t frame_stride, const cilqr_obstacles* obs,
                          const double* obs_cov, uint32_t flags, const double* pose_out, const double* dim_out, const double* cov_out,
                          size_t* span) {
  int rc = check_sizes(h, B, N, M);
  if (rc) return rc;
  rc = frame_stride_check("cilqr_frame_obstacles", frames, frame_stride);
  if (rc) return rc;
  if (flags & ~CILQR_FRAME_GLOBAL_INFLATION) return fail(CILQR_ERR_ARG, "cilqr_frame_obstacles: unknown flag bits 0x%x", flags);
  if (M > 0 && !obs) return fail(CILQR_ERR_ARG, "cilqr_frame_obstacles: M = %d but obs is null", M);
  if (M > 0 && (!pose_out || !dim_out)) return fail(CILQR_ERR_ARG, "cilqr_frame_obstacles: M = %d but pose_out or dim_out is null", M);
  if (M > 0 && !obs_cov != !cov_out) return fail(CILQR_ERR_ARG, "cilqr_frame_obstacles: obs_cov and cov_out must be given together");
  if (M > 0 && obs && (obs->batch_stride < 0 || obs->obstacle_stride < 0 || obs->step_stride < 0))
    return fail(CILQR_ERR_ARG, "cilqr_frame_obstacles: negative stride in obs");
  cilqr_obstacles o = M > 0 && obs ? *obs : cilqr_obstacles{};
  o.weight = nullptr; o.weight_batch_stride = 0;  // not read
  return check_obstacles(B, N, M, M > 0 && obs ? &o : nullptr, span, nullptr);
}

int frame_obstacles_launch(cilqr_handle* h, void* stream, int B, int N, int M, const double* frames, int64_t frame_stride,
                           const cilqr_obstacles& o, const double* obs_cov, uint32_t flags, double* pose_out, double* dim_out,
                           double* cov_out) {
  cilqr::FrameObstaclesArgs a = {};
  a.frames = frames; a.pose = o.pose; a.dim = o.dim; a.cov = obs_cov;
  a.pose_out = pose_out; a.dim_out = dim_out; a.cov_out = cov_out;
  a.bs = o.batch_stride; a.ms = o.obstacle_stride; a.ts = o.step_stride;
  a.two_t_safe = 2.0 * h->kp.t_safe;
  a.B = B; a.N = N; a.M = M; a.frame_stride = (int32_t)frame_stride; a.flags = flags;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_frame_obstacles(a, (hipStream_t)stream));
  return CILQR_OK;
}

int frame_states_check(const cilqr_handle* h, int B, int S, int N, const double* frames, int64_t frame_stride, int direction,
                       const double* X_in, const double* X_out) {
  int rc = check_sizes(h, B, N, 0);
  if (rc) return rc;
  rc = frame_stride_check("cilqr_frame_states", frames, frame_stride);
  if (rc) return rc;
  if (S < 1 || (int64_t)B * S > h->max_batch)
    return fail(CILQR_ERR_ARG, "cilqr_frame_states: S=%d: B*S must be in [0,%d] and S at least 1", S, h->max_batch);
  if (direction != CILQR_FRAME_TO && direction != CILQR_FRAME_FROM)
    return fail(CILQR_ERR_ARG, "cilqr_frame_states: direction=%d is neither CILQR_FRAME_TO nor CILQR_FRAME_FROM", direction);
  if (B > 0 && (!X_in || !X_out)) return fail(CILQR_ERR_ARG, "cilqr_frame_states: X_in or X_out is null");
  return CILQR_OK;
}

int frame_poses_check(const cilqr_handle* h, int B, int K, const double* frames, int64_t frame_stride, const double* pose_in,
                      int64_t pose_stride, const double* pose_out) {
  int rc = check_sizes(h, B, 1, 0);
  if (rc) return rc;
  rc = frame_stride_check("cilqr_frame_poses", frames, frame_stride);
  if (rc) return rc;
  if (K < 1 || (int64_t)B * K > (int64_t)h->max_batch * h->max_horizon)
    return fail(CILQR_ERR_ARG, "cilqr_frame_poses: K=%d: at least 1 and B*K at most %lld", K, (long long)h->max_batch * h->max_horizon);
  if (pose_stride != 0 && pose_stride < 3 * (int64_t)K)
    return fail(CILQR_ERR_ARG, "cilqr_frame_poses: pose_stride=%lld is neither 0 nor at least 3*K", (long long)pose_stride);
  if (B > 0 && (!pose_in || !pose_out)) return fail(CILQR_ERR_ARG, "cilqr_frame_poses: pose_in or pose_out is null");
  return CILQR_OK;
}
}  // namespace

int cilqr_local_plan_frames_device(cilqr_handle* h, void* stream, int B, int P, const double* path, int64_t path_stride,
                                   const double* ego, double* frames, int32_t* info, double* ego_out, double* poly,
                                   double* xplan_fl, double* ref_traj, int32_t* n_out, int32_t* first_out) {
  int rc = local_plan_frames_check(h, B, P, path, path_stride, ego, frames, info, ego_out, poly, xplan_fl);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  cilqr::LocalPlanFramesArgs a = {};
  a.p.path = path; a.p.path_stride = path_stride; a.p.ego = ego;
  a.p.poly = poly; a.p.xplan_fl = xplan_fl; a.p.ref_traj = ref_traj; a.p.n_out = n_out;
  a.p.B = B; a.p.P = P; a.p.n_wpts = h->params.num_of_local_wpts; a.p.cols = h->params.poly_order + 1;
  a.frames = frames; a.info = info; a.ego_out = ego_out; a.first_out = first_out;
  HIP_TRY(cilqr::launch_local_plan_frames(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_local_plan_frames(cilqr_handle* h, int B, int P, const double* path, int64_t path_stride, const double* ego,
                            double* frames, int32_t* info, double* ego_out, double* poly, double* xplan_fl, double* ref_traj,
                            int32_t* n_out, int32_t* first_out) {
  int rc = local_plan_frames_check(h, B, P, path, path_stride, ego, frames, info, ego_out, poly, xplan_fl);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t W = h->params.num_of_local_wpts, b = B;
  const size_t n_path = path_stride ? (size_t)(B - 1) * path_stride + 2 * (size_t)P : 2 * (size_t)P;
  // the scratch slots of cilqr_local_plan_batch; the block of doubles is followed by the three int32 arrays
  void *vp = nullptr, *vio = nullptr;
  rc = cilqr::scratch_bytes(h, cilqr::SCR_PLAN_PATH, n_path * sizeof(double), &vp);
  if (rc) return rc;
  const size_t o_ego = 0, o_poly = o_ego + b * 4, o_fl = o_poly + b * CILQR_POLY_COEFFS, o_ref = o_fl + b * 2, o_fr = o_ref + b * 2 * W,
               o_eo = o_fr + b * CILQR_FRAME_DOUBLES, o_n = o_eo + b * 4;
  rc = cilqr::scratch_bytes(h, cilqr::SCR_PLAN_IO, o_n * sizeof(double) + 3 * b * sizeof(int32_t), &vio);
  if (rc) return rc;
  double* d_path = (double*)vp;
  double* io = (double*)vio;
  int32_t* d_n = (int32_t*)(io + o_n);
  int32_t *d_info = d_n + b, *d_first = d_n + 2 * b;
  hipStream_t s = h->stream;
  if (ref_traj) HIP_TRY(hipMemsetAsync(io + o_ref, 0, b * 2 * W * sizeof(double), s));
  HIP_TRY(hipMemcpyAsync(d_path, path, n_path * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(io + o_ego, ego, b * 4 * sizeof(double), hipMemcpyHostToDevice, s));
  rc = cilqr_local_plan_frames_device(h, s, B, P, d_path, path_stride, io + o_ego, io + o_fr, d_info, io + o_eo, io + o_poly, io + o_fl,
                                      ref_traj ? io + o_ref : nullptr, n_out ? d_n : nullptr, first_out ? d_first : nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(frames, io + o_fr, b * CILQR_FRAME_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(info, d_info, b * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(ego_out, io + o_eo, b * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(poly, io + o_poly, b * CILQR_POLY_COEFFS * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(xplan_fl, io + o_fl, b * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (ref_traj) HIP_TRY(hipMemcpyAsync(ref_traj, io + o_ref, b * 2 * W * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_out) HIP_TRY(hipMemcpyAsync(n_out, d_n, b * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (first_out) HIP_TRY(hipMemcpyAsync(first_out, d_first, b * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CILQR_OK;
}

int cilqr_frame_obstacles_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* frames, int64_t frame_stride,
                                 const cilqr_obstacles* obs, const double* obs_cov, uint32_t flags, double* pose_out,
                                 double* dim_out, double* cov_out) {
  int rc = frame_obstacles_check(h, B, N, M, frames, frame_stride, obs, obs_cov, flags, pose_out, dim_out, cov_out, nullptr);
  if (rc) return rc;
  if (B == 0 || M == 0) return CILQR_OK;
  return frame_obstacles_launch(h, stream, B, N, M, frames, frame_stride, *obs, obs_cov, flags, pose_out, dim_out, cov_out);
}

int cilqr_frame_obstacles(cilqr_handle* h, int B, int N, int M, const double* frames, int64_t frame_stride,
                          const cilqr_obstacles* obs, const double* obs_cov, uint32_t flags, double* pose_out, double* dim_out,
                          double* cov_out) {
  size_t span = 0;
  int rc = frame_obstacles_check(h, B, N, M, frames, frame_stride, obs, obs_cov, flags, pose_out, dim_out, cov_out, &span);
  if (rc) return rc;
  if (B == 0 || M == 0) return CILQR_OK;
  // Not through the arena: a dense table in and out is up to 18·M·N doubles per solve, three times what the arena reserves for
  // one.  The two conversion scratch slots of the handle take it instead (grown on first use, like the pre-step's), so every
  // B <= max_batch fits whatever the strides.
  const size_t b = B, n_out = b * M * N, n_fr = frame_stride ? b * CILQR_FRAME_DOUBLES : (size_t)CILQR_FRAME_DOUBLES;
  const size_t i_pose = n_fr, i_dim = i_pose + span * 4, i_cov = i_dim + span * 2, i_end = i_cov + (obs_cov ? span * 3 : 0);
  const size_t o_dim = n_out * 4, o_cov = o_dim + n_out * 2, o_end = o_cov + (cov_out ? n_out * 3 : 0);
  HIP_TRY(hipSetDevice(h->device));
  void *vin = nullptr, *vout = nullptr;
  rc = cilqr::scratch_bytes(h, cilqr::SCR_CONV_IN, i_end * sizeof(double), &vin);
  if (rc == CILQR_OK) rc = cilqr::scratch_bytes(h, cilqr::SCR_CONV_OUT, o_end * sizeof(double), &vout);
  if (rc) return rc;
  double *in = (double*)vin, *out = (double*)vout;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(in, frames, n_fr * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(in + i_pose, obs->pose, span * 4 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(in + i_dim, obs->dim, span * 2 * sizeof(double), hipMemcpyHostToDevice, s));
  if (obs_cov) HIP_TRY(hipMemcpyAsync(in + i_cov, obs_cov, span * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  cilqr_obstacles o = *obs;
  o.pose = in + i_pose; o.dim = in + i_dim; o.weight = nullptr;
  rc = frame_obstacles_launch(h, s, B, N, M, in, frame_stride, o, obs_cov ? in + i_cov : nullptr, flags, out, out + o_dim,
                              cov_out ? out + o_cov : nullptr);
  if (rc) { (void)hipStreamSynchronize(s); return rc; }
  HIP_TRY(hipMemcpyAsync(pose_out, out, n_out * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(dim_out, out + o_dim, n_out * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (cov_out) HIP_TRY(hipMemcpyAsync(cov_out, out + o_cov, n_out * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CILQR_OK;
}

int cilqr_frame_states_device(cilqr_handle* h, void* stream, int B, int S, int N, const double* frames, int64_t frame_stride,
                              int direction, const double* X_in, double* X_out) {
  int rc = frame_states_check(h, B, S, N, frames, frame_stride, direction, X_in, X_out);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::FrameStatesArgs a = {};
  a.frames = frames; a.X_in = X_in; a.X_out = X_out;
  a.rows = (long long)B * S; a.S = S; a.N = N; a.frame_stride = (int32_t)frame_stride; a.direction = direction;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_frame_states(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_frame_states(cilqr_handle* h, int B, int S, int N, const double* frames, int64_t frame_stride, int direction,
                       const double* X_in, double* X_out) {
  int rc = frame_states_check(h, B, S, N, frames, frame_stride, direction, X_in, X_out);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  const size_t b = B, n = b * S * 4 * ((size_t)N + 1);
  cilqr::HostPlan p(h->d_arena);
  p.in(frames, frame_stride ? b * CILQR_FRAME_DOUBLES : (size_t)CILQR_FRAME_DOUBLES);
  p.in(X_in, n);
  p.out(X_out, n);  // (in place for the caller: two places in the arena)
  return cilqr::host_call(h, p, [&] {
    return cilqr_frame_states_device(h, h->stream, B, S, N, frames, frame_stride, direction, X_in, X_out);
  });
}

int cilqr_frame_poses_device(cilqr_handle* h, void* stream, int B, int K, const double* frames, int64_t frame_stride,
                             const double* pose_in, int64_t pose_stride, double* pose_out) {
  int rc = frame_poses_check(h, B, K, frames, frame_stride, pose_in, pose_stride, pose_out);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  cilqr::FramePosesArgs a = {};
  a.frames = frames; a.pose_in = pose_in; a.pose_out = pose_out;
  a.pose_stride = pose_stride; a.B = B; a.K = K; a.frame_stride = (int32_t)frame_stride;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_frame_poses(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_frame_poses(cilqr_handle* h, int B, int K, const double* frames, int64_t frame_stride, const double* pose_in,
                      int64_t pose_stride, double* pose_out) {
  int rc = frame_poses_check(h, B, K, frames, frame_stride, pose_in, pose_stride, pose_out);
  if (rc) return rc;
  if (B == 0) return CILQR_OK;
  const size_t b = B;
  cilqr::HostPlan p(h->d_arena);
  p.in(frames, frame_stride ? b * CILQR_FRAME_DOUBLES : (size_t)CILQR_FRAME_DOUBLES);
  p.in(pose_in, pose_stride ? (b - 1) * (size_t)pose_stride + 3 * (size_t)K : 3 * (size_t)K);
  p.out(pose_out, b * K * 3);
  return cilqr::host_call(h, p, [&] {
    return cilqr_frame_poses_device(h, h->stream, B, K, frames, frame_stride, pose_in, pose_stride, pose_out);
  });
}

int cilqr_occupancy_to_layer_device(cilqr_handle* h, void* stream, const int8_t* occ, int64_t n_cells, float* layer) {
  if (!h || n_cells < 0 || (n_cells > 0 && (!occ || !layer))) return fail(CILQR_ERR_ARG, "cilqr_occupancy_to_layer: bad argument");
  if (n_cells == 0) return CILQR_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(cilqr::launch_occ_to_layer(occ, layer, (long)n_cells, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_layer_to_occupancy_device(cilqr_handle* h, void* stream, const float* layer, int64_t n_cells, float data_min,
                                    float data_max, int8_t* occ) {
  if (!h || n_cells < 0 || (n_cells > 0 && (!occ || !layer))) return fail(CILQR_ERR_ARG, "cilqr_layer_to_occupancy: bad argument");
  if (n_cells == 0) return CILQR_OK;
  HIP_TRY(hipSetDevice(h->device));
  // the step table is rebuilt on the call's stream; eight slots in rotation keep calls in flight on other streams apart
  float* steps = h->d_occ_steps + 128 * (h->occ_slot++ & 7);
  HIP_TRY(cilqr::launch_layer_to_occ(layer, occ, (long)n_cells, data_min, data_max, steps, (hipStream_t)stream));
  return CILQR_OK;
}

namespace {
// host-buffer conversions: staged through the handle's scratch slots
int convert_host(cilqr_handle* h, const void* in, size_t in_bytes, void* out, size_t out_bytes, bool to_layer, int64_t n, float lo, float hi) {
  HIP_TRY(hipSetDevice(h->device));
  if (n == 0) return CILQR_OK;
  void *d_in = nullptr, *d_out = nullptr;
  int rc = cilqr::scratch_bytes(h, cilqr::SCR_CONV_IN, in_bytes, &d_in);
  if (rc == CILQR_OK) rc = cilqr::scratch_bytes(h, cilqr::SCR_CONV_OUT, out_bytes, &d_out);
  if (rc) return rc;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, s));
  rc = to_layer ? cilqr_occupancy_to_layer_device(h, s, (const int8_t*)d_in, n, (float*)d_out)
                : cilqr_layer_to_occupancy_device(h, s, (const float*)d_in, n, lo, hi, (int8_t*)d_out);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CILQR_OK;
}
}  // namespace

int cilqr_occupancy_to_layer(cilqr_handle* h, const int8_t* occ, int64_t n_cells, float* layer) {
  if (!h || n_cells < 0 || (n_cells > 0 && (!occ || !layer))) return fail(CILQR_ERR_ARG, "cilqr_occupancy_to_layer: bad argument");
  if (n_cells == 0) return CILQR_OK;
  return convert_host(h, occ, (size_t)n_cells, layer, (size_t)n_cells * sizeof(float), true, n_cells, 0.f, 0.f);
}

int cilqr_layer_to_occupancy(cilqr_handle* h, const float* layer, int64_t n_cells, float data_min, float data_max, int8_t* occ) {
  if (!h || n_cells < 0 || (n_cells > 0 && (!occ || !layer))) return fail(CILQR_ERR_ARG, "cilqr_layer_to_occupancy: bad argument");
  if (n_cells == 0) return CILQR_OK;
  return convert_host(h, layer, (size_t)n_cells * sizeof(float), occ, (size_t)n_cells, false, n_cells, data_min, data_max);
}

namespace {
bool good_geom(const cilqr_map_geom* g) { return g->rows >= 1 && g->cols >= 1 && g->res > 0.0; }

// The SOURCE geometry of a warp must carry the lengths setGeometry writes (cilqr_map_geom_set: len = (double)size * res, these
// very bits).  The warp kernels decide most cells from the quotient alone (0 < q < size, costmap_warp.hip cell_estimated) and the
// others as the reference does (t < len AND index < size); the two agree only under this equality, so a hand-filled geometry with
// a shorter length would give cells of one lane's run different answers.  Needs no handle and no device.
int source_geom_lengths(const char* who, const cilqr_map_geom* g) {
  if (!(g->len_x == (double)g->rows * g->res))
    return fail(CILQR_ERR_ARG, "%s: source geometry len_x=%.17g is not rows*res=%.17g (fill it with cilqr_map_geom_set)", who, g->len_x,
                (double)g->rows * g->res);
  if (!(g->len_y == (double)g->cols * g->res))
    return fail(CILQR_ERR_ARG, "%s: source geometry len_y=%.17g is not cols*res=%.17g (fill it with cilqr_map_geom_set)", who, g->len_y,
                (double)g->cols * g->res);
  return CILQR_OK;
}
}  // namespace

int cilqr_costmap_frame_device(cilqr_handle* h, void* stream, const float* global_layer, const cilqr_map_geom* global_geom,
                               const cilqr_map_geom* vehicle_geom, double vx, double vy, double vtheta, const float* bbox,
                               double sigma_x, double sigma_y, double sigma_theta, float* vehicle_layer,
                               float* uncertainty_layer, int8_t* occupancy_out, int64_t* n_out_of_range_dev) {
  if (!h || !global_layer || !global_geom || !vehicle_geom || !vehicle_layer || !uncertainty_layer)
    return fail(CILQR_ERR_ARG, "cilqr_costmap_frame: null argument");
  int rc = cilqr_warp_costmap_device(h, stream, global_layer, global_geom, vehicle_layer, vehicle_geom, vx, vy, vtheta, bbox,
                                     n_out_of_range_dev);
  if (rc) return rc;
  if (vehicle_geom->rows < 1 || vehicle_geom->cols < 1 || !(vehicle_geom->res > 0.0)) return fail(CILQR_ERR_ARG, "cilqr_costmap_frame: bad geometry");
  cilqr::BlurArgs a;
  a.src = vehicle_layer; a.out = uncertainty_layer; a.count_out = nullptr;
  a.occ_out = occupancy_out; a.occ_min = 0.0f; a.occ_den = 100.0f - 0.0f;  // toOccupancyGrid(..., 0, 100, ...) (M/src/local_costmap.cpp:298)
  a.g = *vehicle_geom; a.index = 0;
  a.sin_t = sin(vtheta); a.cos_t = cos(vtheta);
  a.sigma_x = sigma_x; a.sigma_y = sigma_y; a.sigma_theta = sigma_theta;
  HIP_TRY(cilqr::launch_blur(a, (hipStream_t)stream));
  return CILQR_OK;
}

namespace {
// The argument rules the polygon entry points share; they need no handle and no device.
int check_polygons(const char* who, const cilqr_map_geom* g, int n, int V, const double* vertices) {
  if (!g) return fail(CILQR_ERR_ARG, "%s: null geometry", who);
  if (n < 0 || n > CILQR_MAX_POLYGONS) return fail(CILQR_ERR_ARG, "%s: n_polygons=%d outside [0,%d]", who, n, CILQR_MAX_POLYGONS);
  if (V < 3 || V > CILQR_MAX_POLYGON_VERTICES) return fail(CILQR_ERR_ARG, "%s: n_vertices=%d outside [3,%d]", who, V, CILQR_MAX_POLYGON_VERTICES);
  if (n > 0 && !vertices) return fail(CILQR_ERR_ARG, "%s: null vertices", who);
  for (size_t k = 0; k < (size_t)n * V * 2; ++k)
    if (!__builtin_isfinite(vertices[k])) return fail(CILQR_ERR_ARG, "%s: vertex %zu of polygon %zu is not finite", who, (k / 2) % V, k / (2 * (size_t)V));
  if (g->rows < 1 || g->cols < 1 || !(g->res > 0.0)) return fail(CILQR_ERR_ARG, "%s: bad geometry", who);
  return CILQR_OK;
}

// Cells of one axis whose centres c0 - res*i can lie in [lo, hi], widened by one cell and clamped to [0, cells): false if none.
bool cell_range(double c0, double res, int cells, double lo, double hi, int32_t& first, int32_t& last) {
  const double a = floor((c0 - hi) / res) - 1.0, b = ceil((c0 - lo) / res) + 1.0;
  if (!(a <= (double)(cells - 1)) || !(b >= 0.0)) return false;
  first = (int32_t)fmax(a, 0.0);
  last = (int32_t)fmin(b, (double)(cells - 1));
  return true;
}

// The device table of costmap_polygons.hpp for the polygons whose vertex bounding box can touch the map, into the next of the
// handle's slots on stream s.  The ranges are a cull and nothing else: dropping a polygon here is the same cull, made once.
int upload_polygons(cilqr_handle* h, hipStream_t s, const cilqr_map_geom& g, int n, int V, const double* vertices, cilqr::PolygonTable& t) {
  std::vector<int32_t> ranges;
  std::vector<int> kept;
  const double cx0 = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), cy0 = g.pos_y + (0.5 * g.len_y - 0.5 * g.res);
  for (int p = 0; p < n; ++p) {
    const double* v = vertices + (size_t)p * V * 2;
    double xlo = v[0], xhi = v[0], ylo = v[1], yhi = v[1];
    for (int k = 1; k < V; ++k) {
      xlo = fmin(xlo, v[2 * k]); xhi = fmax(xhi, v[2 * k]);
      ylo = fmin(ylo, v[2 * k + 1]); yhi = fmax(yhi, v[2 * k + 1]);
    }
    int32_t r[4];
    if (!cell_range(cx0, g.res, g.rows, xlo, xhi, r[0], r[1]) || !cell_range(cy0, g.res, g.cols, ylo, yhi, r[2], r[3])) continue;
    ranges.insert(ranges.end(), r, r + 4);
    kept.push_back(p);
  }
  t.n = (int32_t)kept.size();
  t.V = V;
  double* d_table = h->d_polys + cilqr::POLYGON_TABLE_DOUBLES * (h->poly_slot++ & 7);
  t.table = d_table;
  if (t.n == 0) return CILQR_OK;
  std::vector<double> table((size_t)t.n * (2 + 2 * V));
  memcpy(table.data(), ranges.data(), ranges.size() * sizeof(int32_t));
  for (int q = 0; q < t.n; ++q) memcpy(&table[2 * (size_t)t.n + (size_t)q * 2 * V], vertices + (size_t)kept[q] * V * 2, sizeof(double) * 2 * V);
  // (pageable source: the runtime has staged the copy by the time the call returns, as with the pose tables below)
  HIP_TRY(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, s));
  return CILQR_OK;
}
}  // namespace

int cilqr_boxes_to_polygons(int n, const double* boxes, double own_x, double own_y, double own_yaw, double inflate, double max_distance,
                            double* vertices, int32_t* n_kept) {
#pragma clang fp contract(off)
  if (n < 0 || !n_kept || (n > 0 && (!boxes || !vertices))) return fail(CILQR_ERR_ARG, "cilqr_boxes_to_polygons: bad argument");
  int32_t kept = 0;
  for (int b = 0; b < n; ++b) {
    const double posX = boxes[5 * b], posY = boxes[5 * b + 1], yaw = boxes[5 * b + 2];
    const double dx = posX - own_x, dy = posY - own_y;
    const double distance = sqrt(dx * dx + dy * dy);  // M/src/local_costmap.cpp:870 (std::pow(d, 2) is d*d)
    if (!(distance <= max_distance)) continue;         // :875
    const double half_x = (boxes[5 * b + 3] + inflate) / 2.0, half_y = (boxes[5 * b + 4] + inflate) / 2.0;  // :880-886
    const double corners[4][2] = {{half_x, half_y}, {half_x, -half_y}, {-half_x, -half_y}, {-half_x, half_y}};  // :889-893
    double* out = vertices + (size_t)kept * 8;
    for (int c = 0; c < 4; ++c) {  // :897-910
      const double global_x = cos(yaw) * corners[c][0] - sin(yaw) * corners[c][1] + posX;
      const double global_y = sin(yaw) * corners[c][0] + cos(yaw) * corners[c][1] + posY;
      out[2 * c] = cos(own_yaw) * (global_x - own_x) + sin(own_yaw) * (global_y - own_y);
      out[2 * c + 1] = -sin(own_yaw) * (global_x - own_x) + cos(own_yaw) * (global_y - own_y);
    }
    ++kept;
  }
  *n_kept = kept;
  return CILQR_OK;
}

int cilqr_rasterize_polygons_device(cilqr_handle* h, void* stream, const cilqr_map_geom* g, int n_polygons, int n_vertices,
                                    const double* vertices, float value, int clear, float* layer) {
  int rc = check_polygons("cilqr_rasterize_polygons", g, n_polygons, n_vertices, vertices);
  if (rc) return rc;
  if (!h || !layer) return fail(CILQR_ERR_ARG, "cilqr_rasterize_polygons: null argument");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->device));
  cilqr::PolygonTable t;
  rc = upload_polygons(h, s, *g, n_polygons, n_vertices, vertices, t);
  if (rc) return rc;
  HIP_TRY(cilqr::launch_rasterize_polygons(t, *g, value, clear != 0, layer, s));
  return CILQR_OK;
}

int cilqr_rasterize_polygons(cilqr_handle* h, const cilqr_map_geom* g, int n_polygons, int n_vertices, const double* vertices,
                             float value, int clear, float* layer) {
  int rc = check_polygons("cilqr_rasterize_polygons", g, n_polygons, n_vertices, vertices);
  if (rc) return rc;
  if (!h || !layer) return fail(CILQR_ERR_ARG, "cilqr_rasterize_polygons: null argument");
  HIP_TRY(hipSetDevice(h->device));
  const size_t cells = (size_t)g->rows * g->cols;
  rc = grow(&h->d_dst, &h->dst_cap, cells);
  if (rc) return rc;
  hipStream_t s = h->stream;
  if (!clear) HIP_TRY(hipMemcpyAsync(h->d_dst, layer, cells * sizeof(float), hipMemcpyHostToDevice, s));
  rc = cilqr_rasterize_polygons_device(h, s, g, n_polygons, n_vertices, vertices, value, clear, h->d_dst);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(layer, h->d_dst, cells * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CILQR_OK;
}

int cilqr_warp_costmap_polygons_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* sg, float* dst,
                                       const cilqr_map_geom* dg, double vx, double vy, double vtheta, int n_polygons, int n_vertices,
                                       const double* vertices, int64_t* n_oob_dev) {
  int rc = check_polygons("cilqr_warp_costmap_polygons", dg, n_polygons, n_vertices, vertices);
  if (rc) return rc;
  if (!h || !src || !sg || !dst) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap_polygons: null argument");
  if (sg->rows < 1 || sg->cols < 1 || !(sg->res > 0.0)) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap_polygons: bad geometry");
  rc = source_geom_lengths("cilqr_warp_costmap_polygons", sg);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->device));
  cilqr::PolygonTable t;
  rc = upload_polygons(h, s, *dg, n_polygons, n_vertices, vertices, t);
  if (rc) return rc;
  cilqr::WarpArgs a;
  a.src = src; a.dst = dst; a.bbox = nullptr;
  a.n_oob = (unsigned long long*)n_oob_dev;
  a.sg = *sg; a.dg = *dg;
  a.vx = vx; a.vy = vy;
  a.sin_t = sin(vtheta);  // host libm, as the reference (M/src/local_costmap.cpp:201-202)
  a.cos_t = cos(vtheta);
  if (n_oob_dev) HIP_TRY(hipMemsetAsync(n_oob_dev, 0, sizeof(int64_t), s));
  HIP_TRY(cilqr::launch_warp_polygons(a, t, s));
  return CILQR_OK;
}

int cilqr_costmap_frame_polygons_device(cilqr_handle* h, void* stream, const float* global_layer, const cilqr_map_geom* global_geom,
                                        const cilqr_map_geom* vehicle_geom, double vx, double vy, double vtheta, int n_polygons,
                                        int n_vertices, const double* vertices, double sigma_x, double sigma_y, double sigma_theta,
                                        float* vehicle_layer, float* uncertainty_layer, int8_t* occupancy_out, int64_t* n_out_of_range_dev) {
  int rc = check_polygons("cilqr_costmap_frame_polygons", vehicle_geom, n_polygons, n_vertices, vertices);
  if (rc) return rc;
  if (!h || !global_layer || !global_geom || !vehicle_layer || !uncertainty_layer)
    return fail(CILQR_ERR_ARG, "cilqr_costmap_frame_polygons: null argument");
  rc = cilqr_warp_costmap_polygons_device(h, stream, global_layer, global_geom, vehicle_layer, vehicle_geom, vx, vy, vtheta, n_polygons,
                                          n_vertices, vertices, n_out_of_range_dev);
  if (rc) return rc;
  cilqr::BlurArgs a;  // as cilqr_costmap_frame_device
  a.src = vehicle_layer; a.out = uncertainty_layer; a.count_out = nullptr;
  a.occ_out = occupancy_out; a.occ_min = 0.0f; a.occ_den = 100.0f - 0.0f;
  a.g = *vehicle_geom; a.index = 0;
  a.sin_t = sin(vtheta); a.cos_t = cos(vtheta);
  a.sigma_x = sigma_x; a.sigma_y = sigma_y; a.sigma_theta = sigma_theta;
  HIP_TRY(cilqr::launch_blur(a, (hipStream_t)stream));
  return CILQR_OK;
}

int cilqr_map_geom_set(cilqr_map_geom* g, double len_x, double len_y, double res, double pos_x, double pos_y) {
  if (!g || !(len_x > 0.0) || !(len_y > 0.0) || !(res > 0.0)) return fail(CILQR_ERR_ARG, "cilqr_map_geom_set: bad argument");
  // GridMap::setGeometry (G/grid_map_core/src/GridMap.cpp:45-62)
  g->rows = (int)round(len_x / res);
  g->cols = (int)round(len_y / res);
  g->res = res;
  g->len_x = (double)g->rows * res;
  g->len_y = (double)g->cols * res;
  g->pos_x = pos_x;
  g->pos_y = pos_y;
  return CILQR_OK;
}

int cilqr_warp_costmap_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* sg, float* dst,
                              const cilqr_map_geom* dg, double vx, double vy, double vtheta, const float* bbox,
                              int64_t* n_oob_dev) {
  if (!h || !src || !sg || !dst || !dg) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap: null argument");
  if (sg->rows < 1 || sg->cols < 1 || dg->rows < 1 || dg->cols < 1 || !(sg->res > 0.0) || !(dg->res > 0.0))
    return fail(CILQR_ERR_ARG, "cilqr_warp_costmap: bad geometry");
  if (int rc = source_geom_lengths("cilqr_warp_costmap", sg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->device));
  cilqr::WarpArgs a;
  a.src = src; a.dst = dst; a.bbox = bbox;
  a.n_oob = (unsigned long long*)n_oob_dev;
  a.sg = *sg; a.dg = *dg;
  a.vx = vx; a.vy = vy;
  a.sin_t = sin(vtheta);  // host libm, as the reference (M/src/local_costmap.cpp:201-202)
  a.cos_t = cos(vtheta);
  if (n_oob_dev) HIP_TRY(hipMemsetAsync(n_oob_dev, 0, sizeof(int64_t), s));
  HIP_TRY(cilqr::launch_warp(a, s));
  return CILQR_OK;
}

namespace {
// The [K][4] device table (vx, vy, sin theta, cos theta) of the batched warp and blur kernels, into the next of the handle's slots
// on stream s.  Frame k's vx, vy and theta are rows[k*stride + ix / iy / it] (ix < 0: no translation, zeros).
int upload_pose_table(cilqr_handle* h, hipStream_t s, int K, const double* rows, int stride, int ix, int iy, int it, double** d_out) {
  double table[1024 * 4];
  for (int k = 0; k < K; ++k) {
    const double* r = rows + (size_t)stride * k;
    table[4 * k] = ix < 0 ? 0.0 : r[ix];
    table[4 * k + 1] = ix < 0 ? 0.0 : r[iy];
    table[4 * k + 2] = sin(r[it]);  // host libm, as the reference (M/src/local_costmap.cpp:201-202)
    table[4 * k + 3] = cos(r[it]);
  }
  // eight device slots in rotation keep the tables of calls still in flight (on other streams) apart; the copy itself is
  // staged by the runtime before this call returns (pageable source)
  double* d_table = h->d_poses + (size_t)1024 * 4 * (h->pose_slot++ & 7);
  HIP_TRY(hipMemcpyAsync(d_table, table, sizeof(double) * 4 * K, hipMemcpyHostToDevice, s));
  *d_out = d_table;
  return CILQR_OK;
}

}  // namespace

int cilqr_warp_costmap_batch_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* sg, float* dst,
                                    const cilqr_map_geom* dg, int K, const double* poses, const float* bbox, int64_t* n_oob_dev) {
  if (!h || !src || !sg || !dst || !dg || !poses) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap_batch: null argument");
  if (K < 1 || K > 1024) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap_batch: K=%d outside [1,1024]", K);
  if (sg->rows < 1 || sg->cols < 1 || dg->rows < 1 || dg->cols < 1 || !(sg->res > 0.0) || !(dg->res > 0.0))
    return fail(CILQR_ERR_ARG, "cilqr_warp_costmap_batch: bad geometry");
  if (int rc = source_geom_lengths("cilqr_warp_costmap_batch", sg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->device));
  if (dg->rows % 4 != 0 && K == 1)  // rows not in fours: one frame is the single-frame kernel's, its pose in the arguments
    return cilqr_warp_costmap_device(h, stream, src, sg, dst, dg, poses[0], poses[1], poses[2], bbox, n_oob_dev);
  double* d_table = nullptr;
  int rc = upload_pose_table(h, s, K, poses, 3, 0, 1, 2, &d_table);
  if (rc) return rc;
  if (n_oob_dev) HIP_TRY(hipMemsetAsync(n_oob_dev, 0, sizeof(int64_t) * K, s));
  cilqr::WarpBatchArgs a;
  a.src = src; a.dst = dst; a.bbox = bbox;
  a.n_oob = (unsigned long long*)n_oob_dev;
  a.poses = d_table;
  a.sg = *sg; a.dg = *dg;
  HIP_TRY(cilqr::launch_warp_batch(a, K, s));
  return CILQR_OK;
}

int cilqr_blur_costmap_batch_device(cilqr_handle* h, void* stream, const float* src, int64_t src_stride, const cilqr_map_geom* g,
                                    int index, int K, const double* vthetas, double sigma_x, double sigma_y, double sigma_theta,
                                    float* out, int32_t* count_out) {
  if (!h || !src || !g || !vthetas || !out) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap_batch: null argument");
  if (K < 1 || K > 1024) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap_batch: K=%d outside [1,1024]", K);
  if (!good_geom(g) || index < 0) return fail(CILQR_ERR_ARG, "cilqr_blur_costmap_batch: bad geometry");
  const int64_t cells = (int64_t)g->rows * g->cols;
  if (src_stride < 0 || (src_stride > 0 && src_stride < cells))
    return fail(CILQR_ERR_ARG, "cilqr_blur_costmap_batch: src_stride=%lld is neither 0 nor >= rows*cols=%lld", (long long)src_stride, (long long)cells);
  if (K == 1) return cilqr_blur_costmap_device(h, stream, src, g, index, vthetas[0], sigma_x, sigma_y, sigma_theta, out, count_out);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->device));
  double* d_table = nullptr;
  int rc = upload_pose_table(h, s, K, vthetas, 1, -1, -1, 0, &d_table);
  if (rc) return rc;
  cilqr::BlurArgs a;  // as cilqr_blur_costmap_device; sine and cosine come from the table
  a.src = src; a.out = out; a.count_out = count_out;
  a.occ_out = nullptr; a.occ_min = 0.0f; a.occ_den = 100.0f;
  a.g = *g; a.index = index;
  a.sin_t = 0.0; a.cos_t = 0.0;
  a.sigma_x = sigma_x; a.sigma_y = sigma_y; a.sigma_theta = sigma_theta;
  HIP_TRY(cilqr::launch_blur_batch(a, K, d_table, (long)src_stride, s));
  return CILQR_OK;
}

int cilqr_costmap_frame_batch_device(cilqr_handle* h, void* stream, const float* global_layer, const cilqr_map_geom* global_geom,
                                     const cilqr_map_geom* vehicle_geom, int K, const double* poses, const float* bbox,
                                     double sigma_x, double sigma_y, double sigma_theta, float* vehicle_layers,
                                     float* uncertainty_layers, int8_t* occupancy_out, int64_t* n_out_of_range_dev) {
  if (!h || !global_layer || !global_geom || !vehicle_geom || !poses || !vehicle_layers || !uncertainty_layers)
    return fail(CILQR_ERR_ARG, "cilqr_costmap_frame_batch: null argument");
  if (K < 1 || K > 1024) return fail(CILQR_ERR_ARG, "cilqr_costmap_frame_batch: K=%d outside [1,1024]", K);
  if (!good_geom(global_geom) || !good_geom(vehicle_geom)) return fail(CILQR_ERR_ARG, "cilqr_costmap_frame_batch: bad geometry");
  if (int rc = source_geom_lengths("cilqr_costmap_frame_batch", global_geom)) return rc;
  if (K == 1)
    return cilqr_costmap_frame_device(h, stream, global_layer, global_geom, vehicle_geom, poses[0], poses[1], poses[2], bbox, sigma_x, sigma_y,
                                      sigma_theta, vehicle_layers, uncertainty_layers, occupancy_out, n_out_of_range_dev);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(h->device));
  double* d_table = nullptr;  // one table for both launches: the warp reads all four entries of a row, the blur its sine and cosine
  int rc = upload_pose_table(h, s, K, poses, 3, 0, 1, 2, &d_table);
  if (rc) return rc;
  if (n_out_of_range_dev) HIP_TRY(hipMemsetAsync(n_out_of_range_dev, 0, sizeof(int64_t) * K, s));
  cilqr::WarpBatchArgs w;
  w.src = global_layer; w.dst = vehicle_layers; w.bbox = bbox;
  w.n_oob = (unsigned long long*)n_out_of_range_dev;
  w.poses = d_table;
  w.sg = *global_geom; w.dg = *vehicle_geom;
  HIP_TRY(cilqr::launch_warp_batch(w, K, s));
  cilqr::BlurArgs a;  // as cilqr_costmap_frame_device, frame k blurring the vehicle layer the warp has just written for it
  a.src = vehicle_layers; a.out = uncertainty_layers; a.count_out = nullptr;
  a.occ_out = occupancy_out; a.occ_min = 0.0f; a.occ_den = 100.0f - 0.0f;
  a.g = *vehicle_geom; a.index = 0;
  a.sin_t = 0.0; a.cos_t = 0.0;
  a.sigma_x = sigma_x; a.sigma_y = sigma_y; a.sigma_theta = sigma_theta;
  HIP_TRY(cilqr::launch_blur_batch(a, K, d_table, (long)vehicle_geom->rows * vehicle_geom->cols, s));
  return CILQR_OK;
}

int cilqr_warp_costmap(cilqr_handle* h, const float* src, const cilqr_map_geom* sg, float* dst, const cilqr_map_geom* dg,
                       double vx, double vy, double vtheta, const float* bbox, int64_t* n_out_of_range) {
  if (!h || !src || !sg || !dst || !dg) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap: null argument");
  if (sg->rows < 1 || sg->cols < 1 || dg->rows < 1 || dg->cols < 1) return fail(CILQR_ERR_ARG, "cilqr_warp_costmap: bad geometry");
  if (int rc0 = source_geom_lengths("cilqr_warp_costmap", sg)) return rc0;  // before the copies below are enqueued
  HIP_TRY(hipSetDevice(h->device));
  const size_t ns = (size_t)sg->rows * sg->cols, nd = (size_t)dg->rows * dg->cols;
  int rc = grow(&h->d_src, &h->src_cap, ns);
  if (rc == CILQR_OK) rc = grow(&h->d_dst, &h->dst_cap, nd);
  if (rc == CILQR_OK && bbox) rc = grow(&h->d_bbox, &h->bbox_cap, nd);
  if (rc) return rc;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(h->d_src, src, ns * sizeof(float), hipMemcpyHostToDevice, s));
  if (bbox) HIP_TRY(hipMemcpyAsync(h->d_bbox, bbox, nd * sizeof(float), hipMemcpyHostToDevice, s));
  rc = cilqr_warp_costmap_device(h, s, h->d_src, sg, h->d_dst, dg, vx, vy, vtheta, bbox ? h->d_bbox : nullptr, (int64_t*)h->d_oob);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(dst, h->d_dst, nd * sizeof(float), hipMemcpyDeviceToHost, s));
  unsigned long long oob = 0;
  HIP_TRY(hipMemcpyAsync(&oob, h->d_oob, sizeof(oob), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (n_out_of_range) *n_out_of_range = (int64_t)oob;
  return CILQR_OK;
}

}  // extern "C"
