// cilqr_track.hip — one tick of the obstacle tracker (cilqr_track_update*, include/cilqr.h): the boxes cilqr_map_obstacles found
// this tick against the track table of the last one — predict, gate, associate, update, retire, start new tracks — and the track,
// track_dim and track_cov rows cilqr_predict_obstacles reads, slot-ordered.
//
// Mapping: one wavefront per world, W workgroups of 64 lanes, one launch.  A world's bits come from its own inputs alone.
//   load     the world's detections and (without CILQR_TRACK_RESET) its state rows enter LDS by coalesced loads; lane = slot m then
//            takes its row from there, so an in-place call has read everything before it stores anything.
//   predict  lane = slot: constant velocity, the ten row <= column entries of P- = F P F' + Q written out for the two non-zero
//            entries of F - I.
//   gate     lane = slot forms S and its determinant once and walks the detections in LDS (every lane reads the same word: a
//            broadcast) keeping its best admissible one that is still unassigned.
//   rounds   greedy global nearest neighbour: the wavefront-wide lexicographic minimum of (d2, m, d) by four DPP steps inside
//            each row of 16 lanes and v_readlane of the four row results — no LDS atomics, no ds_bpermute round trips.  The winner
//            is wave-uniform (scalar registers), so the loop's exit is a scalar branch; at most min(M, D) rounds.  After a round
//            only the lanes whose best detection was taken walk the list again.
//   update   lane = matched slot: gain, state, Joseph form, all 4 x 4 work in registers with constant indices.
//   births   lane = detection: ballots of the unassigned valid detections and of the slots free on entry; the r-th such detection
//            leaves its index in a 64-word LDS list, the slot of rank r picks it up; IDs are NEXT_ID + r.  Counts are popcounts.
//   stores   every lane puts its 32-double state row, then its 24 output doubles, into one [64][33] staging block (33: lanes a row
//            apart fall into different banks), from which the wavefront stores them coalesced.
// LDS (static): detections 2.5 KiB, staging 16.5 KiB, two 64-word lists.  No atomics, no scratch memory, no spilled register
// (make check).  Everything is evaluated as written: no fused multiply-add outside sincos_fast's own.
#include <limits.h>

#include "cilqr_device.hpp"

#pragma clang fp contract(off)

namespace cilqr {

using namespace dev;

namespace {

constexpr int TS = CILQR_TRACK_STATE;
constexpr int ROW = TS + 1;
constexpr int SLOTS = CILQR_TRACK_MAX_SLOTS;
constexpr int KEY_NONE = INT_MAX;  // the (m, d) of a lane with nothing to offer: above every m << 8 | d

// Row <= column entry (r, c) of a symmetric 4x4 in the order 00 01 02 03 11 12 13 22 23 33.
__device__ __forceinline__ constexpr int upper_index(int r, int c) {
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return (lo == 0 ? 0 : lo == 1 ? 3 : lo == 2 ? 5 : 6) + hi;
}

__device__ __forceinline__ bool key_less(double a2, int amd, double b2, int bmd) { return a2 < b2 || (a2 == b2 && amd < bmd); }

template <int CTRL>
__device__ __forceinline__ void key_min_dpp(double& d2, int& md) {
  const int lo = __double2loint(d2), hi = __double2hiint(d2);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  const int omd = __builtin_amdgcn_update_dpp(md, md, CTRL, 0xF, 0xF, false);
  const double o2 = __hiloint2double(ohi, olo);
  const bool take = key_less(o2, omd, d2, md);
  d2 = take ? o2 : d2;
  md = take ? omd : md;
}

// The smallest (d2, md) of the wavefront, wave-uniform.  Every lane must be active.  d2 is never NaN here.
__device__ __forceinline__ void wave_key_min(double& d2, int& md) {
  key_min_dpp<0xB1>(d2, md);   // quad_perm [1, 0, 3, 2]
  key_min_dpp<0x4E>(d2, md);   // quad_perm [2, 3, 0, 1]
  key_min_dpp<0x141>(d2, md);  // row_half_mirror
  key_min_dpp<0x140>(d2, md);  // row_mirror: every lane of a row of 16 now holds the row's minimum
  const int lo = __double2loint(d2), hi = __double2hiint(d2);
  double b2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
  int bmd = __builtin_amdgcn_readlane(md, 0);
#pragma unroll
  for (int l = 16; l < WAVE; l += 16) {
    const double o2 = __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
    const int omd = __builtin_amdgcn_readlane(md, l);
    const bool take = key_less(o2, omd, b2, bmd);
    b2 = take ? o2 : b2;
    bmd = take ? omd : bmd;
  }
  d2 = b2;
  md = bmd;
}

__global__ __launch_bounds__(TRACK_THREADS) void cilqr_track_update_kernel(TrackArgs a) {
  __shared__ double dl[CILQR_TRACK_MAX_DETECTIONS * 5];
  __shared__ double stage[SLOTS * ROW];
  __shared__ int asg[CILQR_TRACK_MAX_DETECTIONS], det_list[CILQR_TRACK_MAX_DETECTIONS];
  const int lane = threadIdx.x, M = a.M, D = a.D;
  const size_t w = blockIdx.x;
  const bool reset = (a.flags & CILQR_TRACK_RESET) != 0;
  const cilqr_track_filter& f = a.f;
  const double inf = __builtin_huge_val();

  int n = D;
  if (a.n_det) {
    n = a.n_det[w * a.n_det_stride];
    n = n < 0 ? 0 : n > D ? D : n;
  }
  {
    const double* det = a.det + w * 5 * D;
    for (int i = lane; i < 5 * n; i += WAVE) dl[i] = det[i];
  }
  double next_id = 0.0, ticks = 0.0;
  if (!reset) {
    const double* in = a.state_in + w * M * TS;
    for (int i = lane; i < M * TS; i += WAVE) stage[(i >> 5) * ROW + (i & (TS - 1))] = in[i];
    next_id = a.world[w * CILQR_TRACK_WORLD_FIELDS + CILQR_TW_NEXT_ID];
    ticks = a.world[w * CILQR_TRACK_WORLD_FIELDS + CILQR_TW_TICKS];
  }
  __syncthreads();

  // ---- the lane's slot
  double s[4] = {0.0, 0.0, 0.0, 0.0}, p[10], sx = 0.0, sy = 0.0, yaw = 0.0, id = -1.0, hits = 0.0, misses = 0.0, age = 0.0, detf = 0.0;
#pragma unroll
  for (int i = 0; i < 10; ++i) p[i] = 0.0;
  bool live = false;
  if (lane < M && !reset) {
    const double* row = stage + lane * ROW;
    live = row[CILQR_TS_ID] >= 0.0;
    if (live) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = row[i];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = r; c < 4; ++c) p[upper_index(r, c)] = row[CILQR_TS_P + r + 4 * c];
      sx = row[CILQR_TS_SIZE_X]; sy = row[CILQR_TS_SIZE_Y]; yaw = row[CILQR_TS_YAW];
      id = row[CILQR_TS_ID]; hits = row[CILQR_TS_HITS]; misses = row[CILQR_TS_MISSES]; age = row[CILQR_TS_AGE];
    }
  }

  // ---- predict
  if (live) {
    const double dt = f.dt;
    s[0] = s[0] + dt * s[2];
    s[1] = s[1] + dt * s[3];
    // G = F P (rows 0 and 1 gain dt times rows 2 and 3), then P- = G F' (columns likewise) + Q
    const double g00 = p[0] + dt * p[2], g01 = p[1] + dt * p[5], g02 = p[2] + dt * p[7], g03 = p[3] + dt * p[8];
    const double g11 = p[4] + dt * p[6], g12 = p[5] + dt * p[8], g13 = p[6] + dt * p[9];
    p[0] = g00 + dt * g02; p[1] = g01 + dt * g03; p[2] = g02; p[3] = g03;
    p[4] = g11 + dt * g13; p[5] = g12; p[6] = g13;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) p[upper_index(r, c)] = p[upper_index(r, c)] + f.Q[r + 4 * c];
    age = age + 1.0;
  }

  // ---- gate
  const double s00 = p[0] + f.R[0], s01 = p[1] + f.R[2], s11 = p[4] + f.R[3];
  const double dets = s00 * s11 - s01 * s01;
  const double gate2 = f.gate2;
  const bool dvalid = lane < n && isfinite(dl[5 * lane]) && isfinite(dl[5 * lane + 1]);
  const unsigned long long vmask = __ballot(dvalid);
  const int invalid = __popcll(__ballot(lane < n && !dvalid));
  asg[lane] = dvalid ? -1 : -2;
  __syncthreads();

  // the lane's best admissible detection among `avail` (wave-uniform: the walk's skips are scalar branches)
  auto scan = [&](unsigned long long avail, double& b2, int& bd) {
    b2 = inf;
    bd = -1;
    for (int d = 0; d < n; ++d) {
      if (!((avail >> d) & 1ull)) continue;
      const double nx = dl[5 * d] - s[0], ny = dl[5 * d + 1] - s[1];
      const double q = (s11 * nx * nx - 2.0 * s01 * nx * ny + s00 * ny * ny) / dets;
      if (q <= gate2 && (bd < 0 || q < b2)) { b2 = q; bd = d; }
    }
  };

  // ---- greedy rounds
  unsigned long long avail = vmask;
  int matched = -1, bd = -1;
  double b2 = inf;
  bool open = live && dets > 0.0;
  if (open) scan(avail, b2, bd);
  for (int round = 0; round < SLOTS; ++round) {
    const bool offer = open && bd >= 0;
    double k2 = offer ? b2 : inf;
    int kmd = offer ? (lane << 8 | bd) : KEY_NONE;
    wave_key_min(k2, kmd);
    if (kmd == KEY_NONE) break;
    const int wm = kmd >> 8, wd = kmd & 255;
    avail &= ~(1ull << wd);
    if (lane == wm) { matched = wd; open = false; asg[wd] = wm; }
    if (open && bd == wd) scan(avail, b2, bd);
  }

  // ---- update, miss, death
  bool died = false;
  if (matched >= 0) {
    const double* dd = dl + 5 * matched;
    const double nx = dd[0] - s[0], ny = dd[1] - s[1];
    double P[4][4], K[4][2], B[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) P[r][c] = p[upper_index(r, c)];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      K[i][0] = (P[i][0] * s11 - P[i][1] * s01) / dets;
      K[i][1] = (P[i][1] * s00 - P[i][0] * s01) / dets;
      s[i] = s[i] + (K[i][0] * nx + K[i][1] * ny);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) B[i][k] = P[i][k] - (K[i][0] * P[0][k] + K[i][1] * P[1][k]);
    const double r00 = f.R[0], r01 = f.R[2], r11 = f.R[3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j)
        p[upper_index(i, j)] = (B[i][j] - (B[i][0] * K[j][0] + B[i][1] * K[j][1])) +
                               (K[i][0] * (r00 * K[j][0] + r01 * K[j][1]) + K[i][1] * (r01 * K[j][0] + r11 * K[j][1]));
    yaw = dd[2]; sx = dd[3]; sy = dd[4];
    hits = hits + 1.0;
    misses = 0.0;
    detf = (double)matched;
  } else if (live) {
    misses = misses + 1.0;
    detf = -1.0;
    died = misses > (double)f.max_misses;
  }
  if (died) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) p[i] = 0.0;
    sx = sy = yaw = hits = misses = age = detf = 0.0;
    id = -1.0;
  }

  // ---- births: lane = detection leaves its index at its rank; lane = slot free on entry takes the one of its own rank
  const bool unassigned = dvalid && ((avail >> lane) & 1ull);
  const unsigned long long ub = __ballot(unassigned), fb = __ballot(lane < M && !live);
  const unsigned long long below = (1ull << lane) - 1ull;
  if (unassigned) det_list[__popcll(ub & below)] = lane;
  const int waiting = __popcll(ub), room = __popcll(fb), born = waiting < room ? waiting : room;
  const int frank = __popcll(fb & below);
  __syncthreads();
  if (lane < M && !live && frank < born) {
    const int d = det_list[frank];
    const double* dd = dl + 5 * d;
    s[0] = dd[0]; s[1] = dd[1]; s[2] = 0.0; s[3] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) p[upper_index(r, c)] = f.P_birth[r + 4 * c];
    yaw = dd[2]; sx = dd[3]; sy = dd[4];
    id = next_id + (double)frank;
    hits = 1.0; misses = 0.0; age = 0.0;
    detf = (double)d;
    asg[d] = lane;
  }
  const bool live_now = lane < M && id >= 0.0;
  const bool confirmed = live_now && hits >= (double)f.min_hits;
  const int n_live = __popcll(__ballot(live_now)), n_conf = __popcll(__ballot(confirmed));
  const int n_matched = __popcll(__ballot(matched >= 0)), n_died = __popcll(__ballot(died));

  // ---- state, assign and the world record
  if (lane < M) {
    double* row = stage + lane * ROW;
#pragma unroll
    for (int i = 0; i < 4; ++i) row[i] = s[i];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) row[CILQR_TS_P + r + 4 * c] = p[upper_index(r, c)];
    row[CILQR_TS_SIZE_X] = sx; row[CILQR_TS_SIZE_Y] = sy; row[CILQR_TS_YAW] = yaw;
    row[CILQR_TS_ID] = id; row[CILQR_TS_HITS] = hits; row[CILQR_TS_MISSES] = misses; row[CILQR_TS_AGE] = age;
    row[CILQR_TS_DET] = detf;
    row[28] = 0.0; row[29] = 0.0; row[30] = 0.0; row[31] = 0.0;
  }
  __syncthreads();
  {
    double* out = a.state_out + w * M * TS;
    for (int i = lane; i < M * TS; i += WAVE) out[i] = stage[(i >> 5) * ROW + (i & (TS - 1))];
    if (a.assign && lane < D) a.assign[w * D + lane] = asg[lane];
    if (lane < CILQR_TRACK_WORLD_FIELDS) {
      const double v = lane == CILQR_TW_NEXT_ID ? next_id + (double)born
                     : lane == CILQR_TW_TICKS   ? ticks + 1.0
                     : (double)(lane == CILQR_TW_LIVE        ? n_live
                                : lane == CILQR_TW_CONFIRMED ? n_conf
                                : lane == CILQR_TW_MATCHED   ? n_matched
                                : lane == CILQR_TW_BORN      ? born
                                : lane == CILQR_TW_DIED      ? n_died
                                : lane == CILQR_TW_DROPPED   ? waiting - born
                                                             : invalid);
      a.world[w * CILQR_TRACK_WORLD_FIELDS + lane] = v;
    }
  }
  __syncthreads();

  // ---- the rows cilqr_predict_obstacles reads: [0, 6) track, [6, 8) dimensions, [8, 24) covariance
  if (lane < M) {
    double* row = stage + lane * ROW;
    double t[6] = {CILQR_MAP_OBSTACLES_FAR, CILQR_MAP_OBSTACLES_FAR, 0.0, 0.0, 0.0, 0.0}, d0 = 0.0, d1 = 0.0, c[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = 0.0;
    if (confirmed) {
      const double vx = s[2], vy = s[3];
      const double v = hypot(vx, vy);
      t[0] = s[0]; t[1] = s[1];
      c[0] = p[0]; c[1] = p[1]; c[4] = p[4];
      if (v >= f.v_min) {
        const double th = atan2(vy, vx);
        t[2] = v; t[3] = th;
        const double ja = vx / v, jb = vy / v, jc = -vy / (v * v), jd = vx / (v * v);
        c[2] = p[2] * ja + p[3] * jb; c[3] = p[2] * jc + p[3] * jd;
        c[5] = p[5] * ja + p[6] * jb; c[6] = p[5] * jc + p[6] * jd;
        const double ea = ja * p[7] + jb * p[8], eb = ja * p[8] + jb * p[9];  // row 0 of Jv Pvv
        const double ec = jc * p[7] + jd * p[8], ed = jc * p[8] + jd * p[9];  // row 1
        c[7] = ea * ja + eb * jb; c[8] = ea * jc + eb * jd; c[9] = ec * jc + ed * jd;
        double sn, cs;
        sincos_fast(th - yaw, &sn, &cs);
        const bool along = fabs(cs) >= fabs(sn);
        d0 = along ? sx : sy;
        d1 = along ? sy : sx;
      } else {
        t[3] = yaw;
        c[7] = p[7] + p[9];
        c[9] = f.theta_var_slow;
        d0 = sx; d1 = sy;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) row[i] = t[i];
    row[6] = d0; row[7] = d1;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) row[8 + r + 4 * cc] = c[upper_index(r, cc)];
  }
  __syncthreads();
  {
    double* tr = a.track_out + w * M * 6;
    for (int i = lane; i < M * 6; i += WAVE) { const int m = i / 6; tr[i] = stage[m * ROW + (i - 6 * m)]; }
    double* dm = a.dim_out + w * M * 2;
    for (int i = lane; i < M * 2; i += WAVE) dm[i] = stage[(i >> 1) * ROW + 6 + (i & 1)];
    double* cv = a.cov_out + w * M * 16;
    for (int i = lane; i < M * 16; i += WAVE) cv[i] = stage[(i >> 4) * ROW + 8 + (i & 15)];
  }
}

}  // namespace

hipError_t launch_track_update(const TrackArgs& a, hipStream_t stream) {
  if (a.W <= 0) return hipSuccess;
  hipLaunchKernelGGL(cilqr_track_update_kernel, dim3((unsigned)a.W), dim3(TRACK_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
