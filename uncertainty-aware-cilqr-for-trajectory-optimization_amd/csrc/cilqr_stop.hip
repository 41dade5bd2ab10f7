// cilqr_stop.hip — stop plans (cilqr_stop_plans*, include/cilqr.h): the geometry of a solved plan under a braking speed profile.
// Row r = b·D + l follows the path of plan b while braking at decel[l]; the definitions — the path as a monotone polyline, the
// acceleration, the pursuit of the path by arc length, the clamp — are the header's, and this file forms them by its statements.
//
// Nothing is summed across rows or plans, and the one sum there is, the running sums of a path, runs on a tree fixed by N (64
// chunks of ceil((N + 1)/64) elements, a doubling scan over the chunk totals): a row's bits depend on its plan, its level, hold and the
// parameters alone, so the mapping is free:
//   path   wavefront = plan.  Lanes take the elements of their chunk in order: sincos of the heading, the clamped advance, the
//          finiteness of every state and control; the scan; then the vertices V_t, the arc lengths s_t, the directions and the
//          plan's own controls go to LDS, PATH_W doubles per step.
//   chain  lane = row, in the workgroup's first wavefront: the state stays in registers over the horizon, and the two segment
//          pointers (the pursuit target's and the deviation's) only move forward, so a row walks its path once.
//   rows   leave as in cilqr_rollout.hip: TILE steps x 64 rows staged in LDS (rows padded by one double), written out by all four
//          wavefronts as whole row segments of 256 bytes (X_stop) and 128 bytes (U_stop).
// How many plans share a workgroup: a plan's path costs one wavefront's pass over it, so with up to STOP_WAVES plans per workgroup
// every path of the workgroup is formed at once and the chain starts no later than with one plan per workgroup, while the planner's
// shape (16 plans x 4 to 8 levels) fills 16 to 32 lanes of the chain's wavefront in place of 4 to 8.  More plans per workgroup would
// fill it further but form their paths one after the other in front of a chain that is latency-bound either way.  More than 64
// levels split into chunks of 64, one plan per workgroup.
// No atomics, no scratch memory; every row index is formed in 64 bits.
#include "cilqr_rollout_core.hpp"

namespace cilqr {

using namespace dev;

namespace {

constexpr int TILE = 8;           // steps staged per write-out
constexpr int XS = 4 * TILE + 1;  // padded row strides of the staging tiles (doubles)
constexpr int US = 2 * TILE + 1;
constexpr int PATH_W = 7;         // doubles per step of a path: V (2), s, cos, sin of the heading, the plan's U (2)

constexpr double PI = 3.14159265358979323846, TWO_PI = 6.28318530717958647692, INV_TWO_PI = 0.15915494309189533577;

// sincos_loop inside its range; an argument beyond it (a lost plan's, or a row's own after a start speed no vehicle has) is taken as 0.
__device__ __forceinline__ void sincos_small(double x, double* sn, double* cs) {
  sincos_loop(fabs(x) < 1.0e6 ? x : 0.0, *sn, *cs);
}

// A running sum over the 64 lanes by doubling: lane i ends with v_0 + ... + v_i.
__device__ __forceinline__ double wave_scan(double v, int lane) {
  for (int o = 1; o < WAVE; o <<= 1) {
    const double u = __shfl_up(v, o, WAVE);
    if (lane >= o) v += u;
  }
  return v;
}

// The path of plan b → `path` ([N + 1][PATH_W]); returns whether the plan is lost (the same in every lane).  Element t <= N adds
// adv_t (cos, sin, 1) to the running sums whose value BEFORE it is (V_t - P_0, s_t); element N, the end of the path, adds nothing.
__device__ __forceinline__ bool build_path(const StopArgs& a, int b, int lane, double* path) {
  const int N = a.N;
  const double* X = a.X + (size_t)b * 4 * ((size_t)N + 1);
  const double* U = a.U + (size_t)b * 2 * (size_t)N;
  const int chunk = (N + WAVE) / WAVE, t0 = lane * chunk, t1 = min(t0 + chunk, N + 1);  // ceil((N + 1)/64) elements a lane
  bool bad = false;
  double ts = 0.0, tx = 0.0, ty = 0.0;
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const bool last = t == N;
    const int tn = last ? t : t + 1, tu = last ? t - 1 : t;  // (N >= 1; the last element reads in bounds and uses neither)
    const double x = X[4 * t], y = X[4 * t + 1], v = X[4 * t + 2], th = X[4 * t + 3];
    const double xn = X[4 * tn], yn = X[4 * tn + 1];
    const double u0 = last ? 0.0 : U[2 * tu], u1 = last ? 0.0 : U[2 * tu + 1];
    bad |= !(is_finite(x) && is_finite(y) && is_finite(v) && fabs(th) < 1.0e6 && is_finite(u0) && is_finite(u1));  // (1e6: the range of sincos_loop)
    double sn, cs;
    sincos_small(th, &sn, &cs);
    const double adv = last ? 0.0 : fmax((xn - x) * cs + (yn - y) * sn, 0.0);
    double* r = path + (size_t)t * PATH_W;
    r[2] = adv;  // (until the scan has run)
    r[3] = cs; r[4] = sn; r[5] = u0; r[6] = u1;
    ts += adv; tx += adv * cs; ty += adv * sn;
  }
  const double is = wave_scan(ts, lane), ix = wave_scan(tx, lane), iy = wave_scan(ty, lane);
  double rs = __shfl_up(is, 1, WAVE), rx = __shfl_up(ix, 1, WAVE), ry = __shfl_up(iy, 1, WAVE);
  if (lane == 0) { rs = 0.0; rx = 0.0; ry = 0.0; }
  const double x0 = X[0], y0 = X[1];
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    double* r = path + (size_t)t * PATH_W;
    const double adv = r[2], cs = r[3], sn = r[4];
    r[0] = x0 + rx; r[1] = y0 + ry; r[2] = rs;
    rs += adv; rx += adv * cs; ry += adv * sn;
  }
  return __ballot(bad) != 0ull;
}

// Q(sigma) of a path whose length is sN; `seg` is the caller's segment pointer, which only moves forward.
__device__ __forceinline__ void path_point(const double* path, int N, double sN, double sigma, int& seg, double& qx, double& qy) {
  const double* r;
  double from;
  if (sigma >= sN) {
    r = path + (size_t)N * PATH_W;
    from = sN;
  } else {
    while (seg < N - 1 && path[(size_t)(seg + 1) * PATH_W + 2] <= sigma) ++seg;
    r = path + (size_t)seg * PATH_W;
    from = r[2];
  }
  qx = r[0] + (sigma - from) * r[3];
  qy = r[1] + (sigma - from) * r[4];
}

// The braking acceleration of a row at speed v: -min(d, v/dt); `stops`: this step ends at rest.
__device__ __forceinline__ double brake(double v, double d, double dt, bool& stops) {
  stops = false;
  if (v == 0.0) return 0.0;
  const double q = v / dt;
  stops = d >= q;
  return stops ? -q : -d;
}

// LDS (dynamic): [paths: plans·(N + 1)·PATH_W][X tile: 64·XS][U tile: 64·US] | int32: [lost per plan: STOP_WAVES]
__global__ __launch_bounds__(STOP_THREADS) void cilqr_stop_plans_kernel(StopArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int N = a.N, D = a.D, P = a.plans;
  const int chunks = (D + WAVE - 1) / WAVE, LV = min(D, WAVE);
  const int g = blockIdx.x / chunks, ck = blockIdx.x - g * chunks;
  const int b0 = g * P, np = min(P, a.B - b0);  // (1 <= np: the grid has ceil(B / P) groups)
  const size_t path_doubles = ((size_t)N + 1) * PATH_W;
  double* paths = lds;
  double* tx = paths + (size_t)P * path_doubles;
  double* tu = tx + WAVE * XS;
  int* lost_flag = reinterpret_cast<int*>(tu + WAVE * US);

  for (int p = wave; p < np; p += STOP_WAVES) {  // (uniform per wavefront)
    const bool lost = build_path(a, b0 + p, lane, paths + (size_t)p * path_doubles);
    if (lane == 0) lost_flag[p] = lost ? 1 : 0;
  }
  __syncthreads();

  // ---- the rows of this workgroup: consecutive in the output, lane = row in the first wavefront
  const int n_rows = chunks > 1 ? min(WAVE, D - ck * WAVE) : np * D;  // (at most 64: P·LV <= 64)
  const long long row0 = (long long)b0 * D + (long long)ck * WAVE;
  const bool active = lane < n_rows;
  const int p = active ? lane / LV : 0;                        // a lane without a row repeats the first row and stores nothing
  const int l = ck * WAVE + (active ? lane - p * LV : 0);      // (< D)
  const double* path = paths + (size_t)p * path_doubles;
  const StopArgs& kp = kernel_args<StopArgs>();  // (the model's constants, loaded where they are used)
  const double dt = kp.dt, qnan = __builtin_nan("");

  double d = 0.0, sN = 0.0, acc_b = 0.0;  // acc_b: the braking acceleration of the step about to be taken
  bool lost = false, stops = false;
  State st = {};
  if (wave == 0) {
    d = a.decel[l];
    lost = lost_flag[p] != 0 || !(d > 0.0 && d <= -kp.acc_min);
    sN = path[(size_t)N * PATH_W + 2];
    const double* X0 = a.X + (size_t)(b0 + p) * 4 * ((size_t)N + 1);
    st.x = X0[0]; st.y = X0[1]; st.v = X0[2]; st.th = X0[3];
    st.c = path[3]; st.s = path[4];
    acc_b = brake(st.v, d, dt, stops);
  }
  const double inv_dt = 1.0 / dt;
  double sigma = 0.0, dev = -1.0;
  int seg_t = 0, seg_d = 0, stop_step = -1, dev_step = -1, clamped = 0, overrun = 0;

  for (int i0 = 0; i0 <= N; i0 += TILE) {
    const int n_st = min(TILE, N + 1 - i0), n_u = min(TILE, N - i0);  // states i0 … and controls i0 … of this tile (n_u may be 0)
    if (wave == 0) {
      double* mx = tx + lane * XS;
      double* mu = tu + lane * US;
#pragma unroll 1
      for (int ii = 0; ii < n_st; ++ii) {
        const int j = i0 + ii;
        mx[4 * ii] = lost ? qnan : st.x; mx[4 * ii + 1] = lost ? qnan : st.y; mx[4 * ii + 2] = lost ? qnan : st.v; mx[4 * ii + 3] = lost ? qnan : st.th;
        if (st.v == 0.0 && stop_step < 0) stop_step = j;
        {
          double qx, qy;
          path_point(path, N, sN, sigma, seg_d, qx, qy);
          const double ex = st.x - qx, ey = st.y - qy, e = sqrt(ex * ex + ey * ey);
          if (e > dev) { dev = e; dev_step = j; }
        }
        if (j < N) {
          const double* r = path + (size_t)j * PATH_W;
          const bool held = j < a.hold;
          const double u0 = held ? r[5] : acc_b;
          double u1 = held ? r[6] : 0.0;
          // Model::forward_simulate (dyn_step of cilqr_device.hpp), with the speed of the stopping step exactly 0
          const double acc = fmax(fmin(u0, kp.acc_max), kp.acc_min);
          const double adv = st.v * dt + acc * kp.half_dt2;
          State n;
          n.x = st.x + st.c * adv;
          n.y = st.y + st.s * adv;
          n.v = !held && stops ? 0.0 : fmin(fmax(st.v + acc * dt, 0.0), kp.speed_max);
          sigma += fmax(adv, 0.0);
          acc_b = brake(n.v, d, dt, stops);  // (decided here: the next step's advance is what this step aims by)
          if (!held && j < N - 1) {
            const double adv_n = n.v * dt + acc_b * kp.half_dt2;
            if (adv_n >= CILQR_STOP_MIN_ADVANCE) {
              const double target = sigma + adv_n;
              if (target >= sN) ++overrun;
              double qx, qy;
              path_point(path, N, sN, target, seg_t, qx, qy);
              const double turn = atan2(qy - n.y, qx - n.x) - st.th;
              u1 = (turn - TWO_PI * ceil((turn - PI) * INV_TWO_PI)) * inv_dt;
            }
          }
          const double w = fmax(fmin(u1, st.v * kp.yaw_hi), st.v * kp.yaw_lo);
          if (!held) {
            if (w != u1) ++clamped;
            u1 = w;
          }
          mu[2 * ii] = lost ? qnan : u0; mu[2 * ii + 1] = lost ? qnan : u1;
          n.th = st.th + w * dt;
          sincos_small(n.th, &n.s, &n.c);
          st = n;
        }
      }
    }
    __syncthreads();
    // whole row segments: 4·TILE (2·TILE) consecutive lanes on consecutive doubles of one row
    {
      const int c = tid & (4 * TILE - 1), sub = tid / (4 * TILE), step = STOP_THREADS / (4 * TILE);
      double* Xr = a.X_stop + row0 * 4 * ((long long)N + 1) + 4 * i0 + c;
      if (c < 4 * n_st)
        for (int r = sub; r < n_rows; r += step) Xr[(long long)r * 4 * ((long long)N + 1)] = tx[r * XS + c];
    }
    {
      const int c = tid & (2 * TILE - 1), sub = tid / (2 * TILE), step = STOP_THREADS / (2 * TILE);
      double* Ur = a.U_stop + row0 * 2 * (long long)N + 2 * i0 + c;
      if (c < 2 * n_u)
        for (int r = sub; r < n_rows; r += step) Ur[(long long)r * 2 * (long long)N] = tu[r * US + c];
    }
    __syncthreads();
  }

  if (wave == 0 && active) {
    const long long row = row0 + lane;
    double* out = a.sp + row * CILQR_STOP_FIELDS;
    out[CILQR_SP_STOP_STEP] = lost ? -1.0 : (double)stop_step;
    out[CILQR_SP_DISTANCE] = lost ? qnan : sigma;
    out[CILQR_SP_END_SPEED] = lost ? qnan : st.v;
    out[CILQR_SP_DEVIATION] = lost ? qnan : dev;
    out[CILQR_SP_DEVIATION_STEP] = lost ? -1.0 : (double)dev_step;
    out[CILQR_SP_CLAMPED_STEPS] = lost ? 0.0 : (double)clamped;
    out[CILQR_SP_OVERRUN_STEPS] = lost ? 0.0 : (double)overrun;
    out[CILQR_SP_LOST] = lost ? 1.0 : 0.0;
    if (a.cost) {
      const bool at_rest = stop_step >= 0 && stop_step <= N - 1;
      const bool ok = !lost && dev <= a.max_deviation && (at_rest || (a.flags & CILQR_STOP_ALLOW_MOVING));
      a.cost[row] = ok ? a.decel_weight * d + (a.plan_cost ? a.plan_cost[b0 + p] : 0.0) : qnan;
    }
  }
}

static_assert(STOP_THREADS % (4 * TILE) == 0 && STOP_THREADS == STOP_WAVES * WAVE, "a row segment of a tile is dealt to whole groups of lanes");

constexpr size_t STOP_FIXED_BYTES = (size_t)WAVE * (XS + US) * sizeof(double) + STOP_WAVES * sizeof(int32_t);

// one plan's path at the largest horizon a handle accepts, the staging tiles and the flags fit the LDS a launch gets without opting in
static_assert(((size_t)CILQR_MAX_HORIZON + 1) * PATH_W * sizeof(double) + STOP_FIXED_BYTES <= STOP_LDS_MAX, "a path at CILQR_MAX_HORIZON does not fit");

size_t stop_lds_bytes(int N, int plans) { return (size_t)plans * ((size_t)N + 1) * PATH_W * sizeof(double) + STOP_FIXED_BYTES; }

}  // namespace

int stop_plans_per_group(int N, int D) {
  const size_t path = ((size_t)N + 1) * PATH_W * sizeof(double);
  const size_t fit = (STOP_LDS_MAX - STOP_FIXED_BYTES) / path;
  const size_t lanes = (size_t)(WAVE / (D < WAVE ? D : WAVE));  // plans whose rows fit the chain's wavefront (D >= 33: one)
  size_t plans = fit < lanes ? fit : lanes;
  if (plans > (size_t)STOP_WAVES) plans = STOP_WAVES;
  return (int)plans;
}

hipError_t launch_stop_plans(const StopArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.N <= 0 || a.plans <= 0) return hipSuccess;
  const long long blocks = (long long)((a.B + a.plans - 1) / a.plans) * ((a.D + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(cilqr_stop_plans_kernel, dim3((unsigned)blocks), dim3(STOP_THREADS), stop_lds_bytes(a.N, a.plans), stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
