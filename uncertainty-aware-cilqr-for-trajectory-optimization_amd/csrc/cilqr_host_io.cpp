// cilqr_host_io.cpp — the one transport of the host-buffer entry points: how a call's arrays, given in host memory, reach the
// `_device` form of the same call and how its results come back.  SURVEY §8(b) "Ownership": the caller owns every host buffer, the
// library owns device buffers sized at create (host_arena_bytes, cilqr_host_plan.h) and allocates nothing per call.
//
// A host form checks its arguments, declares its arrays in a HostPlan (cilqr_host_plan.h: inputs, then in/out arrays, then
// outputs, each at the next 16-byte-aligned place of the handle's device arena) and hands the plan and its `_device` call to
// host_enqueue / host_call.  Obstacles given by strides travel as the span of entries the strides address.
//   * a call whose plan fits the handle's pinned staging buffer (≤ 1 MiB: the drop-in B = 1 tick, run_candidates, a gains or
//     risk call on a handful of solves): the inputs are packed into pinned memory and travel as ONE host→device copy of the
//     prefix [0, in_end); the results return as ONE device→host copy of the suffix [out_begin, end) and are unpacked after the
//     wait — 2 DMA transfers, each of which costs ≈10 µs of latency whatever its size;
//   * a larger call: each array is copied straight from / to the caller's memory; from memory of cilqr_host_alloc (pinned)
//     these are true asynchronous DMA transfers, from pageable memory the runtime stages them.
// One call per handle is in flight at a time.  Whatever fails once a copy may be in flight, the stream is drained before the
// error returns — no copy to or from the CALLER's memory is left behind — and the handle is free for the next call.
#include <string.h>

#include "cilqr_handle.h"

using cilqr::fail;

namespace cilqr {

namespace {
// The way out of a failed call: the first error's message survives the wait.
int drain(cilqr_handle* h, int rc) {
  const std::string msg = g_last_error;
  (void)hipStreamSynchronize(h->stream);
  h->pending.active = false;
  g_last_error = msg;
  return rc;
}
}  // namespace

int host_copy_in(cilqr_handle* h, const HostPlan& p, bool solve) {
  if (h->pending.active) return fail(CILQR_ERR_ARG, "a host-buffer solve is in flight on this handle");
  if (!p.ok) return fail(CILQR_ERR_ARG, "internal: malformed host plan");
  if (p.end > h->arena_cap) return fail(CILQR_ERR_ARG, "batch does not fit the device buffers reserved at create");
  HIP_TRY(hipSetDevice(h->device));
  hipError_t e = hipSuccess;
  if (p.end <= h->stage_cap) {
    for (int i = 0; i < p.n; ++i)
      if (p.e[i].src) memcpy(h->stage + p.e[i].off, p.e[i].src, p.e[i].bytes);
    if (p.in_end) e = hipMemcpyAsync(h->d_arena, h->stage, p.in_end, hipMemcpyHostToDevice, h->stream);
  } else {
    for (int i = 0; i < p.n && e == hipSuccess; ++i)
      if (p.e[i].src) e = hipMemcpyAsync(h->d_arena + p.e[i].off, p.e[i].src, p.e[i].bytes, hipMemcpyHostToDevice, h->stream);
  }
  if (e != hipSuccess) return drain(h, fail(CILQR_ERR_HIP, "host-buffer call: copy to the device failed: %s", hipGetErrorString(e)));
  if (solve && h->debug_fail_enqueue > 0 && --h->debug_fail_enqueue == 0)  // test hook (cilqr_debug_fail_enqueue): fail with the copies in flight
    return drain(h, fail(CILQR_ERR_HIP, "forced failure after the input copies were enqueued (cilqr_debug_fail_enqueue)"));
  return CILQR_OK;
}

int host_copy_out(cilqr_handle* h, const HostPlan& p, int launch_rc) {
  if (launch_rc != CILQR_OK) return drain(h, launch_rc);
  PendingOut& q = h->pending;
  q.packed = p.end <= h->stage_cap;
  q.n = 0;
  hipError_t e = hipSuccess;
  for (int i = 0; i < p.n; ++i)
    if (p.e[i].dst) q.out[q.n++] = p.e[i];
  if (q.packed) {
    if (p.end > p.out_begin) e = hipMemcpyAsync(h->stage + p.out_begin, h->d_arena + p.out_begin, p.end - p.out_begin, hipMemcpyDeviceToHost, h->stream);
  } else {
    for (int i = 0; i < q.n && e == hipSuccess; ++i)
      e = hipMemcpyAsync(q.out[i].dst, h->d_arena + q.out[i].off, q.out[i].bytes, hipMemcpyDeviceToHost, h->stream);
  }
  if (e != hipSuccess) return drain(h, fail(CILQR_ERR_HIP, "host-buffer call: copy from the device failed: %s", hipGetErrorString(e)));
  q.active = true;
  return CILQR_OK;
}

int host_finish(cilqr_handle* h) {
  PendingOut& q = h->pending;
  if (!q.active) return CILQR_OK;
  q.active = false;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (q.packed)
    for (int i = 0; i < q.n; ++i) memcpy(q.out[i].dst, h->stage + q.out[i].off, q.out[i].bytes);
  return CILQR_OK;
}

// Device scratch of the convenience entry points that take host pointers (local plan, blur counts, conversions, test hooks):
// slots owned by the handle, grown when a call needs more than any before it — never allocated and freed per call.
int scratch_bytes(cilqr_handle* h, int slot, size_t bytes, void** out) {
  *out = nullptr;
  if (bytes == 0) return CILQR_OK;
  if (bytes > h->scratch_cap[slot]) {
    HIP_TRY(hipStreamSynchronize(h->stream));  // nothing enqueued may still use the old block
    if (h->scratch[slot]) HIP_TRY(hipFree(h->scratch[slot]));
    h->scratch[slot] = nullptr;
    h->scratch_cap[slot] = 0;
    const size_t want = bytes + bytes / 4;  // head-room: a slowly growing request does not reallocate every call
    HIP_TRY(hipMalloc(&h->scratch[slot], want));
    h->scratch_cap[slot] = want;
  }
  *out = h->scratch[slot];
  return CILQR_OK;
}

}  // namespace cilqr

extern "C" {

void* cilqr_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    fail(CILQR_ERR_HIP, "cilqr_host_alloc: hipHostMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return p;
}

int cilqr_debug_fail_enqueue(cilqr_handle* h, int nth_call) {
  if (!h || nth_call < 0) return fail(CILQR_ERR_ARG, "cilqr_debug_fail_enqueue: bad argument");
  h->debug_fail_enqueue = nth_call;
  return CILQR_OK;
}

int cilqr_host_free(void* p) {
  if (p) HIP_TRY(hipHostFree(p));
  return CILQR_OK;
}

}  // extern "C"
