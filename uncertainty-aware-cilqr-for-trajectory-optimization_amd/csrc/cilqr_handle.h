// cilqr_handle.h — the handle behind the C-ABI, shared by the translation units that implement include/cilqr.h
// (cilqr_api.cpp: solver / costmap entry points; cilqr_comm.cpp: the RCCL exchange step).  Not installed.
#pragma once

#include <string>

#include "cilqr_host_plan.h"
#include "cilqr_internal.h"

struct ncclComm;  // RCCL communicator (rccl.h), only named here

struct cilqr_handle;

namespace cilqr {
// The transport of every host-buffer call (cilqr_host_io.cpp): the arrays a HostPlan names are copied into the arena, `launch`
// — the call's `_device` form on h->stream with the arena pointers the plan handed out — runs, the outputs are copied back.
// All of it is enqueued by host_enqueue; host_finish waits and, for a call that travelled packed, unpacks the staging buffer.
// What host_finish needs of a call in flight:
struct PendingOut {
  bool active, packed;
  int n;
  HostPlan::Entry out[HostPlan::CAP];  // the entries with a host destination
};
int host_copy_in(cilqr_handle* h, const HostPlan& p, bool solve);  // the two halves of host_enqueue, around the launch
int host_copy_out(cilqr_handle* h, const HostPlan& p, int launch_rc);
int host_finish(cilqr_handle* h);
// `solve`: the call counts for cilqr_debug_fail_enqueue.  On failure the stream is drained and the handle is free again.
template <typename Launch>
int host_enqueue(cilqr_handle* h, const HostPlan& p, Launch&& launch, bool solve = false) {
  const int rc = host_copy_in(h, p, solve);
  return rc ? rc : host_copy_out(h, p, launch());
}
template <typename Launch>
int host_call(cilqr_handle* h, const HostPlan& p, Launch&& launch, bool solve = false) {
  const int rc = host_enqueue(h, p, launch, solve);
  return rc ? rc : host_finish(h);
}
// cilqr_solve_batch, cilqr_solve_batch_obstacles and the shards of cilqr_multi_solve_batch (cilqr_api.cpp): arguments checked by
// the caller, obs = host pointers and strides (null when M == 0) addressing `span` entries and `w_span` weights.  Enqueues only.
int host_solve_enqueue(cilqr_handle* h, int B, int N, int M, const double* x0, double* U, const double* poly, const double* xplan_fl,
                       const cilqr_obstacles* obs, size_t span, size_t w_span, double* X_out, double* J_out, int32_t* iters_out,
                       int32_t* status_out, uint32_t flags);
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
  int debug_fail_enqueue;  // test hook: the n-th host-buffer solve enqueued from now fails after its input copies (0: off)
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
  double* d_chance_map_steps;  // per-step values of cilqr_chance_risk_map the caller did not ask for: 3 x max_batch x max_horizon doubles
  double* d_tighten_map_part;  // workgroup records of cilqr_tighten_map: max_batch x TIGHTEN_MAP_MAX_G x TIGHTEN_MAP_REC doubles
  double* d_track_map_rec;   // entry records of cilqr_rasterize_tracks: max_batch x max_obstacles x max_horizon x TRACK_MAP_ENTRY doubles
  double* d_track_map_part;  // its workgroup records: max_batch x TRACK_MAP_MAX_G x TRACK_MAP_REC doubles
  double* d_footprint_steps;  // step and row records of cilqr_footprint_check: footprint_scratch_doubles(max_batch, max_horizon)
  double* d_chance_sampled_steps;  // step records of cilqr_chance_risk_sampled: CHANCE_SAMPLED_REC x max_batch x max_horizon doubles
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
  double unc_res;  // the set map's resolution as given (unc holds its inverse); read by cilqr_tighten_map
  float* d_unc_layer;
  size_t unc_layer_cap;
  // cross-rank min-cost exchange (cilqr_comm.cpp)
  ncclComm* comm;            // null: this handle is its own world
  int comm_ranks, comm_rank;
  double* d_triple;          // {J_min, local index, index offset} of this rank
  double* d_gather;          // comm_ranks triples
};
