// obstacle_table.hip — the obstacle table of a batch that shares one scene (cilqr_solve_batch_obstacles* with batch stride 0).
// The kernels that keep their table in device memory instead of LDS (the grouped family, cilqr_solve_groups.hip, and the
// one-wavefront kernel past its LDS budget, cilqr_solve.hip with TAB = 0) would otherwise each build an M·N·48-byte copy per solve
// and stream it from HBM on every pass.  Built here once per launch, in front of the solve kernels on the same stream, it is one
// table that stays in L2 for the whole batch.  Every row is filled, those of horizon-constant obstacles included: the production
// kernels read row 0 of a held obstacle, the GENERAL kernels row t.
#include "cilqr_device.hpp"

namespace cilqr {

using namespace dev;

// one lane per entry (m, t) of solve 0 → obs_tab[(m*N + t)*6 …]
__global__ __launch_bounds__(256) void obstacle_table_kernel(SolveArgs a) {
  const int n = a.M * a.N;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int m = i / a.N;
    const ObsEntry e = obs_entry_at(a.kp, a, 0, m, i - m * a.N);
    double2* o = reinterpret_cast<double2*>(a.obs_tab + (size_t)i * TABF);
    o[0] = make_double2(e.ox, e.oy);
    o[1] = make_double2(e.co, e.so);
    o[2] = make_double2(e.ia2, e.ib2);
  }
}

hipError_t launch_obstacle_table(const SolveArgs& a, hipStream_t stream) {
  const int n = a.M * a.N;
  if (n <= 0) return hipSuccess;
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(obstacle_table_kernel, dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
