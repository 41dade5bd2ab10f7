// cilqr_frame.hip — what surrounds a solve in a path-aligned planning frame (include/cilqr.h): the obstacle rows, map poses
// and states of a batch taken into the frames the framed pre-step chose (local_plan.hip), and states taken back out.  The solve,
// score, gains, risk and check kernels read what these write and do not know of the frame.
//
// Mapping: one lane per element — obstacle entry (b, m, t), state (row, step) or pose (b, k) — in the order of the dense output,
// so that the lanes of a wavefront read and write neighbouring 16- to 32-byte records (coalesced).  Each lane loads its solve's
// five frame doubles itself (40 bytes that the lanes of a solve share: a cache line or two per wavefront).  No LDS, no scratch
// memory, nothing carried between lanes.  Every product and sum is rounded on its own (cilqr_frame.hpp): the tests compare bits.
#include "cilqr_device.hpp"
#include "cilqr_frame.hpp"

namespace cilqr {

using frame::Frame;

namespace {
constexpr int FRAME_BLOCK = 256;

__device__ __forceinline__ Frame frame_of(const double* frames, int frame_stride, long long b) {
  return frame::load_frame(frames + b * frame_stride);
}
}  // namespace

// lane i = (b·M + m)·N + t of the dense output
__global__ __launch_bounds__(FRAME_BLOCK) void frame_obstacles_kernel(FrameObstaclesArgs a) {
#pragma clang fp contract(off)
  const long long total = (long long)a.B * a.M * a.N;
  const long long i = (long long)blockIdx.x * FRAME_BLOCK + threadIdx.x;
  if (i >= total) return;
  const long long bm = i / a.N;
  const int t = (int)(i - bm * a.N);
  const long long b = bm / a.M;
  const int m = (int)(bm - b * a.M);
  const Frame f = frame_of(a.frames, a.frame_stride, b);
  const long long e = b * a.bs + (long long)m * a.ms + (long long)t * a.ts;
  const double* pin = a.pose + 4 * e;
  const double ox = pin[0], oy = pin[1], v = pin[2], th = pin[3];
  double L = a.dim[2 * e], W = a.dim[2 * e + 1];
  double xf, yf;
  frame::point_to(f, ox, oy, &xf, &yf);
  const double thf = th - f.phi;
  double* pout = a.pose_out + 4 * i;
  pout[0] = xf;
  pout[1] = yf;
  pout[2] = v;
  pout[3] = thf;
  if (a.flags & CILQR_FRAME_GLOBAL_INFLATION) {
    // the solver will add |v·cos θ'|·t_safe and |v·sin θ'|·t_safe to the semi-axes: hand it what makes those sums the map frame's
    double sg, cg, sf, cf;
    dev::sincos_fast(th, &sg, &cg);
    dev::sincos_fast(thf, &sf, &cf);
    const double da = fabs(v * cg) - fabs(v * cf);
    const double db = fabs(v * sg) - fabs(v * sf);
    L = L + a.two_t_safe * da;
    W = W + a.two_t_safe * db;
  }
  a.dim_out[2 * i] = L;
  a.dim_out[2 * i + 1] = W;
  if (a.cov_out) {  // T C Tᵀ, T = (c s; −s c): first T C, then times Tᵀ
    const double cxx = a.cov[3 * e], cxy = a.cov[3 * e + 1], cyy = a.cov[3 * e + 2];
    const double m00 = f.c * cxx + f.s * cxy, m01 = f.c * cxy + f.s * cyy;
    const double m10 = f.c * cxy - f.s * cxx, m11 = f.c * cyy - f.s * cxy;
    a.cov_out[3 * i] = m00 * f.c + m01 * f.s;
    a.cov_out[3 * i + 1] = m01 * f.c - m00 * f.s;
    a.cov_out[3 * i + 2] = m11 * f.c - m10 * f.s;
  }
}

// lane i = row·(N + 1) + t
__global__ __launch_bounds__(FRAME_BLOCK) void frame_states_kernel(FrameStatesArgs a) {
#pragma clang fp contract(off)
  const long long total = a.rows * (a.N + 1);
  const long long i = (long long)blockIdx.x * FRAME_BLOCK + threadIdx.x;
  if (i >= total) return;
  const long long row = i / (a.N + 1);
  const Frame f = frame_of(a.frames, a.frame_stride, row / a.S);
  const double* in = a.X_in + 4 * i;
  const double sx = in[0], sy = in[1], v = in[2], sth = in[3];
  double x, y, th;
  if (a.direction == CILQR_FRAME_TO) {
    frame::point_to(f, sx, sy, &x, &y);
    th = sth - f.phi;
  } else {
    frame::point_from(f, sx, sy, &x, &y);
    th = sth + f.phi;
  }
  double* out = a.X_out + 4 * i;
  out[0] = x;
  out[1] = y;
  out[2] = v;
  out[3] = th;
}

// lane i = b·K + k
__global__ __launch_bounds__(FRAME_BLOCK) void frame_poses_kernel(FramePosesArgs a) {
#pragma clang fp contract(off)
  const long long total = (long long)a.B * a.K;
  const long long i = (long long)blockIdx.x * FRAME_BLOCK + threadIdx.x;
  if (i >= total) return;
  const long long b = i / a.K;
  const int k = (int)(i - b * a.K);
  const Frame f = frame_of(a.frames, a.frame_stride, b);
  const double* in = a.pose_in + b * a.pose_stride + 3 * k;
  const double px = in[0], py = in[1], pth = in[2];
  double x, y;
  frame::point_to(f, px, py, &x, &y);
  double* out = a.pose_out + 3 * i;
  out[0] = x;
  out[1] = y;
  out[2] = pth - f.phi;
}

namespace {
inline unsigned frame_blocks(long long total) { return (unsigned)((total + FRAME_BLOCK - 1) / FRAME_BLOCK); }
}  // namespace

hipError_t launch_frame_obstacles(const FrameObstaclesArgs& a, hipStream_t stream) {
  const long long total = (long long)a.B * a.M * a.N;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(frame_obstacles_kernel, dim3(frame_blocks(total)), dim3(FRAME_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_frame_states(const FrameStatesArgs& a, hipStream_t stream) {
  const long long total = a.rows * (a.N + 1);
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(frame_states_kernel, dim3(frame_blocks(total)), dim3(FRAME_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_frame_poses(const FramePosesArgs& a, hipStream_t stream) {
  const long long total = (long long)a.B * a.K;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(frame_poses_kernel, dim3(frame_blocks(total)), dim3(FRAME_BLOCK), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
