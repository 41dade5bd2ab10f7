// cilqr_handle.h — the handle behind the C-ABI, shared by the translation units that implement include/cilqr.h
// (cilqr_api.cpp: solver / costmap entry points; cilqr_comm.cpp: the RCCL exchange step).  Not installed.
#pragma once

#include <string>

#include "cilqr_internal.h"

struct ncclComm;  // RCCL communicator (rccl.h), only named here

struct cilqr_handle;

namespace cilqr {
// Where a host-buffer call's arrays lie in the handle's device arena and pinned staging buffer (cilqr_host_io.cpp); bytes.
struct IoLayout {
  size_t x0, poly, xplan, obs_w, samp_off, obs_pose, obs_dim, U, X, J, iters, status, end;
};
// obs_entries: obstacle entries (4 pose + 2 dimension doubles each); w_entries: weights; samp_entries: sample-offset records (3 doubles)
IoLayout io_layout(size_t B, size_t N, size_t obs_entries, size_t w_entries, size_t samp_entries);
// One host-buffer solve call (M = obstacles, or nominal obstacles of the sampled form when n_samples > 0).
struct HostBatch {
  int B, N, M, n_samples;
  const double *x0;
  double* U;
  const double *poly, *xplan_fl, *obs_pose, *obs_dim, *obs_weight, *samp_off;
  double samp_w;
  double *X_out, *J_out;
  int32_t *iters_out, *status_out;
  uint32_t flags;
  // cilqr_solve_batch_obstacles: obstacles by strides (entries), of which only the span travels; false: the dense [B][M][N] layout
  bool strided;
  int64_t obs_bs, obs_ms, obs_ts, obs_wbs;
  size_t obs_span, w_span;  // entries and weights the strides address
};
struct PendingOut {
  bool active, packed;
  IoLayout L;
  HostBatch q;
};
int host_solve_enqueue(cilqr_handle* h, const HostBatch& q);  // copies in, kernels, copies out: all enqueued on h->stream
int host_solve_finish(cilqr_handle* h);                       // waits; unpacks the staging buffer of a small call
// One host-buffer score call (cilqr_score_batch, cilqr_score_batch_sampled): synchronous, through the solve's arena and pinned
// staging buffer with a layout of its own (X and U both travel in; the scores and totals come back).
struct HostScore {
  int B, N, M, n_samples;  // M: obstacles, or nominal obstacles of the sampled form (n_samples > 0)
  const double *X, *U, *poly, *xplan_fl;
  cilqr_obstacles obs;     // host pointers; sampled: pose / dim are the dense nominal tables, strides unused
  size_t obs_span, w_span; // entries and weights that travel
  const double* samp_off;
  double samp_w, max_collision;
  double *score, *total;   // total may be null
};
struct ScoreLayout {
  size_t poly, xplan, obs_w, samp_off, obs_pose, obs_dim, U, X, score, total, end;  // inputs poly … X, outputs score, total
};
ScoreLayout score_layout(size_t B, size_t N, size_t obs_entries, size_t w_entries, size_t samp_entries);
int host_score(cilqr_handle* h, const HostScore& q);
enum { SCR_PLAN_PATH, SCR_PLAN_IO, SCR_COUNT, SCR_CONV_IN, SCR_CONV_OUT, SCR_DEBUG, SCR_SLOTS };
int scratch_bytes(cilqr_handle* h, int slot, size_t bytes, void** out);

extern thread_local std::string g_last_error;
int fail(int code, const char* fmt, ...);  // records the message for cilqr_last_error() and returns `code`
}  // namespace cilqr

#define HIP_TRY(expr)                                                                                      \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) return cilqr::fail(CILQR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct cilqr_handle {
  cilqr_params params;
  cilqr::KParams kp;
  int device;
  cilqr::SolveKnobs knobs;  // SIMDs of the device and the environment's A/B and test hooks, read once at create (cilqr_wave_plan.h)
  int max_batch, max_horizon, max_obstacles;
  hipStream_t stream;
  // host-buffer entry points (cilqr_host_io.cpp): device arena and pinned staging sized at create, the call in flight
  char* d_arena;
  size_t arena_cap;
  char* stage;
  size_t stage_cap;
  cilqr::PendingOut pending;
  int debug_fail_enqueue;  // test hook: the n-th host-buffer enqueue from now fails after its input copies (0: off)
  double* d_J;  // the costs of the last host-buffer call, inside the arena
  void* scratch[cilqr::SCR_SLOTS];
  size_t scratch_cap[cilqr::SCR_SLOTS];
  // workspace
  double* d_obs_tab;
  double* d_ws;      // workspace of the G-lanes-per-solve kernel family
  int32_t* d_redo;
  // schedule hint of the one-wavefront-per-solve family: passes of the previous call and the dispatch order built from them
  int32_t* d_hint_passes;
  int32_t* d_order;
  int hint_B;          // batch size the order is valid for (0: none)
  void* hint_stream;   // stream it was built on (a call on another stream does not use it)
  double* d_pair;
  double* d_risk_part;      // partial records of cilqr_rollout_risk: max_batch x risk_part_stride doubles (cilqr_risk.hip)
  size_t risk_part_stride;  // 8 + ceil(max_horizon / 2)
  // warp staging (grown on demand by the host-pointer warp entry point only)
  float *d_src, *d_dst, *d_bbox;
  size_t src_cap, dst_cap, bbox_cap;
  unsigned long long* d_oob;
  double* d_poses;       // 8 slots x 1024 poses x 4 doubles: pose tables of the batched warp / blur / frame calls in flight
  unsigned pose_slot;
  double* d_polys;       // 8 slots x one full polygon table (costmap_polygons.hpp): tables of the polygon calls in flight
  unsigned poly_slot;
  float* d_occ_steps;  // 8 x 128 floats: step tables of the layer -> occupancy conversion (rebuilt per call on the call's stream)
  unsigned occ_slot;
  unsigned long long* diag;  // caller-owned device buffer or null
  int32_t* passes;           // caller-owned device buffer or null (cilqr_set_pass_count_buffer)
  // uncertainty map (cilqr_set_uncertainty_map*): what the kernels read, and the device copy made from a host layer
  cilqr::UncArgs unc;
  float* d_unc_layer;
  size_t unc_layer_cap;
  // cross-rank min-cost exchange (cilqr_comm.cpp)
  ncclComm* comm;            // null: this handle is its own world
  int comm_ranks, comm_rank;
  double* d_triple;          // {J_min, local index, index offset} of this rank
  double* d_gather;          // comm_ranks triples
};
