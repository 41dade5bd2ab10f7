// cilqr_rollout.hip — S closed-loop rollouts per solve from offset starts (cilqr_rollout_batch*, include/cilqr.h): the rollout step
// defined in cilqr_rollout_core.hpp, every state and every control (unclamped) stored.
//
// Mapping: lane = sample.  A workgroup is ONE wavefront holding up to 64 samples of ONE solve, so the nominal X_t, U_t, k_t, K_t are
// the same for every lane: the block copies them to LDS once ({X_t(4), U_t + k_scale·k_t (2), K_t(8)} per step) and every lane
// reads the same address (a broadcast), instead of 64 identical vector loads from global memory per step.  A lane's state stays in
// registers over the whole horizon.
// Stores: a lane's output row is contiguous in memory, so lanes storing their own step would write at a stride of 4(N+1) doubles —
// 64 separate 32-byte pieces per instruction.  Instead TILE steps × 64 lanes are staged in LDS (rows padded by one double: lanes
// then hit different banks) and written out as whole row segments: TILE = 8 makes a segment 256 bytes of X_roll (two full 128-byte
// lines when aligned) and 128 bytes of U_roll per row, with 32 / 16 lanes on consecutive addresses.  A larger tile lengthens the
// segments no further than a line pair is worth and costs LDS linearly (TILE = 8: 25.5 KiB of staging, five workgroups per CU);
// a smaller one cuts the U segment below a line.
// A wavefront whose share of S is partial (S = 70: 64 + 6) computes its idle lanes on a zero offset and stores nothing for them.
// Every row index is formed in 64 bits.  A row depends on its own inputs alone: the same bits whatever B, S and its position.
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int TILE = 8;               // steps staged per write-out
constexpr int XS = 4 * TILE + 1;      // padded row strides of the staging tiles (doubles)
constexpr int US = 2 * TILE + 1;

// LDS (dynamic): [nominal: N·NOM_W + 4 (X_N)][X tile: 64·XS][U tile: 64·US]
__global__ __launch_bounds__(WAVE) void cilqr_rollout_kernel(RolloutArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, N = a.N, S = a.S;
  const int chunks = (S + WAVE - 1) / WAVE;
  const int b = blockIdx.x / chunks, s0 = (blockIdx.x - b * chunks) * WAVE;
  const int n_rows = min(WAVE, S - s0);  // rows of this wavefront
  const bool active = lane < n_rows;
  double* nom = lds;
  double* tx = nom + (size_t)N * NOM_W + 4;
  double* tu = tx + WAVE * XS;

  // ---- the nominal trajectory and gains of solve b → LDS: load_nominal of cilqr_rollout_core.hpp, written out (through the call
  // this launch measured 1.3 % slower, profiles/r16_rollout_core.txt)
  {
    const double* X = a.X + (size_t)b * 4 * (N + 1);
    const double* U = a.U + (size_t)b * 2 * N;
    const double* k = a.k + (size_t)b * 2 * N;
    const double* K = a.K + (size_t)b * 8 * N;
    const double ks = a.k_scale;
    for (int t = lane; t < N; t += WAVE) {
      double* r = nom + (size_t)t * NOM_W;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = X[4 * t + i];
      r[4] = U[2 * t] + ks * k[2 * t];
      r[5] = U[2 * t + 1] + ks * k[2 * t + 1];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[6 + i] = K[8 * (size_t)t + i];
    }
    if (lane < 4) nom[(size_t)N * NOM_W + lane] = X[4 * N + lane];
  }
  __syncthreads();
  State st = start_state(kernel_args<RolloutArgs>(), nom, b, s0 + lane, active);
  const long long row0 = (long long)b * S + s0;  // first row of this wavefront
  double* Xr = a.X_roll + row0 * 4 * (N + 1);
  double* Ur = a.U_roll + row0 * 2 * N;

  // ---- TILE states (and the controls leaving them) at a time
  for (int i0 = 0; i0 <= N; i0 += TILE) {
    const int n_st = min(TILE, N + 1 - i0), n_u = min(TILE, N - i0);  // states i0 … and controls i0 … of this tile (n_u may be 0)
    {
      const KParams& kp = kernel_args<RolloutArgs>().kp;
      double* mx = tx + lane * XS;
      double* mu = tu + lane * US;
      for (int ii = 0; ii < n_st; ++ii) {
        const int i = i0 + ii;
        mx[4 * ii] = st.x; mx[4 * ii + 1] = st.y; mx[4 * ii + 2] = st.v; mx[4 * ii + 3] = st.th;
        if (i < N) {
          const double* r = nom + (size_t)i * NOM_W;
          const double e0 = st.x - r[0], e1 = st.y - r[1], e2 = st.v - r[2], e3 = st.th - r[3];
          // (feedback_control of cilqr_rollout_core.hpp, written out: the form that measured no slower than before)
          const double f0 = fma(r[12], e3, fma(r[10], e2, fma(r[8], e1, r[6] * e0)));
          const double f1 = fma(r[13], e3, fma(r[11], e2, fma(r[9], e1, r[7] * e0)));
          const double u0 = r[4] + f0, u1 = r[5] + f1;
          mu[2 * ii] = u0; mu[2 * ii + 1] = u1;
          st = dyn_step(kp, st, u0, u1);
        }
      }
    }
    __syncthreads();
    // whole row segments: 4·TILE (2·TILE) consecutive lanes on consecutive doubles of one row
    {
      const int c = lane & (4 * TILE - 1), sub = lane / (4 * TILE), step = WAVE / (4 * TILE);
      if (c < 4 * n_st)
        for (int r = sub; r < n_rows; r += step) Xr[(long long)r * 4 * (N + 1) + 4 * i0 + c] = tx[r * XS + c];
    }
    {
      const int c = lane & (2 * TILE - 1), sub = lane / (2 * TILE), step = WAVE / (2 * TILE);
      if (c < 2 * n_u)
        for (int r = sub; r < n_rows; r += step) Ur[(long long)r * 2 * N + 2 * i0 + c] = tu[r * US + c];
    }
    __syncthreads();
  }
}

static_assert(WAVE % (4 * TILE) == 0 && 4 * TILE <= WAVE, "a row segment of the X tile is dealt to whole groups of lanes");

}  // namespace

size_t rollout_lds_bytes(int N) { return ((size_t)N * NOM_W + 4 + (size_t)WAVE * (XS + US)) * sizeof(double); }

hipError_t launch_rollout(const RolloutArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  const long long blocks = (long long)a.B * ((a.S + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(cilqr_rollout_kernel, dim3((unsigned)blocks), dim3(WAVE), rollout_lds_bytes(a.N), stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
