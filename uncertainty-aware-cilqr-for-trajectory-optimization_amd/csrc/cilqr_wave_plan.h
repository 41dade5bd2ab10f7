// cilqr_wave_plan.h — which kernel a batch runs on, with how many wavefronts per solve, with its obstacle table where and with how
// much LDS: one pure host function of the batch shape and the handle's knobs.  cilqr_api.cpp builds the plan, launch_solve_wave
// (cilqr_solve.hip) carries it out, the queries of include/cilqr.h return its fields.  Plain C++17 without HIP (tests/test_wave_plan.py
// runs it where there is no GPU); also the one definition of the record widths the LDS sizes and the kernels are built from.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "cilqr.h"

namespace cilqr {
namespace dev {
constexpr int WAVE = 64;
constexpr int XR = 6;    // doubles per state record {x, y, v, theta, cos theta, sin theta}
constexpr int REC = 16;  // doubles per linearisation record
constexpr int TABF = 6;  // fields per obstacle-table entry
constexpr int RECF = REC - 2;  // record width of the production kernel: p and q are not stored (they are (dt/2)·al, (dt/2)·be)
// Constant table behind the records: {0, 1, dt, 2·w_vel, 2} twice, RECF doubles apart — a lane that reads a constant keeps its
// address while the others step through the records, and the two steps of one loop trip are read at immediate offsets 0 and RECF.
// (Records of 16 doubles would hold p and q, but a lane stride of 128 bytes puts phase L's record stores on two banks only:
// measured +17 % on phase L; 112 bytes spread a quarter-wave's 16-byte stores over all 64 banks.)
constexpr int RCST = REC + 6;
// sampled obstacles (cilqr_solve.hip, SampledObstacles): nominal records in the workspace, offset records in LDS
constexpr int NOMF = 8;  // x, y, cos, sin, v·t_safe, half-length + margins, half-width + margins, pad
constexpr int OFFF = 6;  // dx, dy, then (cos, sin of the SAMPLE's heading, 1/a², 1/b²) for an obstacle of constant shape, else (cos dtheta, sin dtheta, -, -)
// control words behind the per-solve arrays of the kernels with further wavefronts per solve
constexpr int PAIR_CTL = 4;   // doubles: {J of the trajectory in LDS, command | abort (two int32), -, -}
constexpr int SHARE_CTL = 4;  // doubles: {command word, dmax, curvature bound, -}
constexpr int SPLIT_CTL = 2;  // doubles: command word
}  // namespace dev

struct SolveKnobs {  // what cilqr_create reads from the environment, once per handle (read_knobs, cilqr_api.cpp), and the size of the device
  int simds;          // SIMDs of the device (4 per CU): 1024 on an MI355X
  int force_g;        // 0 = automatic; else 1,2,4,8,16,32 or 64 (test hook: CILQR_FORCE_G)
  int hint_off;       // CILQR_NO_SCHEDULE_HINT
  int pair_on;        // CILQR_PAIR_KERNEL: the two-wavefront kernel up to one solve per SIMD (a measured negative result, DESIGN.md §5: kept for the A/B of tools/pair_ab.py)
  int steal_off;      // CILQR_NO_LANE_SHARING: the grouped family without phase L's lane sharing (A/B, bit-equality test)
  int split_off;      // CILQR_NO_SPLIT_KERNEL: sampled obstacles on one wavefront per solve (A/B, tests)
  int split_w;        // 0 = automatic; else 2 or 4 (test hook: CILQR_SPLIT_W)
  int share_off;      // CILQR_NO_SHARE_KERNEL: static obstacles on one wavefront per solve at every batch size (A/B, tests)
  int share_w;        // 0 = automatic (three wavefronts up to three quarters of a solve per SIMD, two beyond); else 2 or 3 (CILQR_SHARE_W)
  int share_max;      // -1: the largest batch on the shared-phase-L kernel follows the horizon (share_wavefronts); CILQR_SHARE_MAX_B overrides
  int tab_budget_kb;  // 0 = automatic (lds_table_budget); else KiB (CILQR_LDS_TABLE_KB: A/B)
};

struct WaveShape {  // one call of the one-wavefront-per-solve family
  int B, N, M;       // M: obstacles; nominal obstacles of the sampled form
  int n_samples;     // pose samples per nominal obstacle; 0 = static obstacles
  int path_samples;  // KParams::n_samples: ordinates of the local path held in LDS
  uint32_t flags;    // CILQR_FLAG_*
  bool has_map, obs_shared;  // an uncertainty map is set; one obstacle scene for the whole batch (SolveArgs::obs_shared)
};
struct WavePlan {
  // launched first: cilqr_solve_kernel, _pair_kernel, _share_kernel or _split_kernel; the GENERAL cilqr_solve_kernel behind it takes the solves it hands over
  enum Kernel { ONE, PAIR, SHARE, SPLIT } kernel;
  int W;               // wavefronts per solve of that kernel
  bool long_form;      // SHARE: two steps per lane (horizons 65 … 127)
  int tab;             // obstacle entries: 0 table in the workspace, 1 table in LDS, 2 sampled (offset records in LDS)
  bool shared_table;   // launch_obstacle_table first: the batch's one scene, read from the workspace by both kernels
  size_t lds_fast, lds_general;  // dynamic LDS per solve of the first kernel and of the GENERAL kernel behind it, bytes
  bool hinted;         // the schedule hint applies (cilqr_api.cpp, launch_wave_scheduled)
  bool too_large;      // a solve of this shape does not fit the LDS of a CU: nothing can be launched
};
constexpr size_t SOLVE_LDS_MAX = 160 * 1024;     // LDS of one CU: the horizon bound of the wavefront family
constexpr size_t SOLVE_LDS_DEFAULT = 64 * 1024;  // dynamic LDS a kernel may take without its limit being raised

// ---- LDS per solve, by kernel: what the carve-up at the top of each kernel adds up to -------------------------------------------
// Bytes of the per-solve arrays: `compact` = the production kernel without CILQR_FLAG_FAITHFUL_ITERS (forward pass in place,
// no candidate buffers); otherwise with candidate buffers.
inline size_t core_lds_bytes(int N, int path_samples, bool compact) {
  const size_t traj = (size_t)(N + 1) * dev::XR + (size_t)2 * N;
  const size_t doubles = (((size_t)path_samples + 1) & ~(size_t)1) + (compact ? 1 : 2) * traj + (size_t)N * (compact ? dev::RECF : dev::REC) + dev::RCST;  // gains overlay the records
  return doubles * sizeof(double);
}
// `extra` behind them, the same for both kernels of a launch: the [M][N] entry table of static obstacles when it lies in LDS, or the
// offset records + rmax + constant-shape flags of sampled obstacles (whose nominal records take sampled_tab_doubles of obs_tab per solve)
inline size_t table_lds_bytes(int N, int M) { return (size_t)M * dev::TABF * N * sizeof(double); }
inline size_t sampled_lds_bytes(int n_obs, int n_samples) { return ((size_t)n_obs * n_samples * dev::OFFF + (size_t)2 * n_obs) * sizeof(double); }
inline size_t sampled_tab_doubles(int n_obs, int N) { return (size_t)n_obs * dev::NOMF * N; }
// share / split kernels: five partial sums per step for every further wavefront, one more set with a map
inline size_t part_doubles(int N, int W, bool unc) { return ((size_t)((W - 1) + (unc ? 1 : 0)) * 5 * N + 1) & ~(size_t)1; }
// cilqr_solve_kernel (the GENERAL instantiation: compact = false), cilqr_solve_pair_kernel, cilqr_solve_share_kernel, cilqr_solve_split_kernel
inline size_t one_lds_bytes(int N, int S, bool compact, size_t extra) { return core_lds_bytes(N, S, compact) + extra; }
inline size_t pair_lds_bytes(int N, int S, size_t extra) { return core_lds_bytes(N, S, true) + extra + ((((size_t)N + 1) & ~(size_t)1) + dev::PAIR_CTL) * sizeof(double); }
inline size_t share_lds_bytes(int N, int S, int W, bool unc, size_t extra) { return core_lds_bytes(N, S, true) + extra + (part_doubles(N, W, unc) + dev::SHARE_CTL) * sizeof(double); }
inline size_t split_lds_bytes(int N, int S, int W, bool unc, size_t extra) { return core_lds_bytes(N, S, true) + extra + (part_doubles(N, W, unc) + dev::SPLIT_CTL) * sizeof(double); }

// Kernel family by batch shape: lanes per solve, 64 = the one-wavefront-per-solve family (cilqr_solve.hip), less =
// the grouped family (cilqr_solve_groups.hip).  Drawn from tools/family_shapes.py (profiles/r03_family_shapes.txt: both families
// at N = 30 … 160, M = 0 … 16, B = 2048 … 16384, first calls, i.e. WITHOUT the schedule hint — on a planner's tick sequence
// the hint changes nothing, profiles/r03_schedule_hint_ticks.txt) and tools/group_lanes_sweep.py.  Up to one solve per SIMD the
// wavefront family always (its backward pass on the matrix cores and scalar-path forward pass give it the shorter serial chain);
// beyond, it keeps batches of a few solves per SIMD while a solve is short — the shorter the horizon and the fewer the
// obstacles, the longer — and the grouped family, whose phase L shares the lanes of finished solves since round 3, takes the
// rest.  Very long horizons (N > 110: the records no longer fit the grouped family's LDS chunks well) stay on the wavefront
// family at every size measured.
inline int plan_group_lanes(const SolveKnobs& k, int B, int N, int M) {
  const int f = k.force_g;
  if (f == 1 || f == 2 || f == 4 || f == 8 || f == 16 || f == 32 || f == 64) return f;
  // (with hundreds of obstacle entries per step the solve is a stream over its obstacle table: the wavefront-per-solve
  // family reads it as whole 400-640 B rows per instruction and measures ≈2x faster there — BASELINE config 3)
  if (M > 32 || N > 110) return 64;
  // largest batch that stays on the wavefront family, in half solves per SIMD
  int cap2;
  // (redrawn at the end of round 3, when the family had got its shared-phase-L kernel up to two solves per SIMD and N = 127:
  // profiles/r03_family_shapes.txt)
  if (N <= 32) cap2 = 16;
  else if (N <= 56) cap2 = 8;
  else if (N <= 92) cap2 = 4;
  else cap2 = 8;
  if (2L * B <= (long)cap2 * k.simds) return 64;
  int G = 32;
  while (G > 1 && (long)G * B > 64L * k.simds) G >>= 1;
  // not below 2 lanes per solve (4 for horizons beyond one round of lanes): with the lanes of finished solves helping in phase L
  // twice as many, smaller wavefronts — started as the first ones end — beat one wavefront per SIMD with 64 solves and 3-step
  // hand-over chunks each (profiles/r03_group_lanes_sweep.txt: B = 65536, N = 50: G = 2 5.7 ms against 7.1 at G = 1; N = 80:
  // G = 4 16.4-19.6 ms against 20.5-24.6)
  const int g_min = N > 64 ? 4 : 2;
  if (G < g_min) G = g_min;
  return G;
}

// Sampled obstacles: wavefronts per solve that share phase L (cilqr_solve_split_kernel), by shape alone: four up to one solve per
// SIMD, where a shorter pass is all that counts, two beyond (tools/split_ab.py, profiles/r03_split_kernel.txt: B = 256
// 0.88 / 1.35 / 2.08 ms with 4 / 2 / 1 wavefronts, B = 1024 1.47 / 1.55 / 2.11, B = 4096 3.86 / 3.27 / 3.97, B = 8192 6.81 / 5.48 / 5.68);
// 1 where the kernel is not built for the shape (N > 64, fewer obstacles than wavefronts).  This is what cilqr_solve_sampled_wavefronts
// answers; plan_wave further falls back to one wavefront in the reference-loop mode and where the kernel's LDS would pass 64 KiB.
inline int split_shape_wavefronts(const SolveKnobs& k, int B, int N, int n_obs) {
  const int w = k.split_off ? 0 : k.split_w ? k.split_w : (B <= k.simds ? 4 : 2);
  if (w < 2 || N > dev::WAVE || n_obs < w) return 1;
  return w >= 4 ? 4 : 2;
}

// Static obstacles on the one-wavefront family: further wavefronts per solve for phase L (cilqr_solve_share_kernel) up to about two solves
// per SIMD — tools/share_ab.py, profiles/r03_share_kernel.txt: config-2 scenes 0.372 against 0.404 ms at B = 256, 0.390 / 0.415 at 1024,
// 0.406 / 0.433 at 2048, level at 3072, slower at 4096 (0.547 / 0.476: the second wavefronts cost residency there).
// Up to THREE QUARTERS of a solve per SIMD three: the obstacle terms on two of them (even / odd entries: obstacle_loop's own two chains),
// Jacobians and control barrier on the last — the solves that decide such a launch are the ones with every obstacle close (B = 256: 0.356
// against 0.362 ms).  Not at one solve per SIMD: three wavefronts of 153 registers fill a SIMD, so a CU holds exactly its four workgroups
// and every unevenness of the dispatch makes one wait for a whole solve (rocprofv3, 61 launches at B = 1024: 395 µs average, 538 µs
// maximum with three; 391 / 418 with two).  0: one wavefront.
inline int share_wavefronts(const SolveKnobs& k, int B, int N, int M, bool has_map) {
  // how far beyond one solve per SIMD the further wavefronts pay depends on how many workgroups a CU still holds, i.e. on the horizon
  // (tools/share_ab.py with CILQR_SHARE_MAX_B open, profiles/r03_share_kernel.txt, last section: N = 30 still 6 % ahead at four solves
  // per SIMD, N = 40 8 % at three, N = 50 8 % at two and level at three, N = 56 / 60 5 / 3 % at 1.5 and behind at two, N = 64 ahead at
  // 1.25 and behind at 1.5, N = 80 2 % at one) — in quarters of a solve per SIMD:
  const int q = N <= 32 ? 16 : N <= 44 ? 12 : N <= 52 ? 8 : N <= 60 ? 6 : N <= 64 ? 5 : 4;
  const long cap = k.share_max >= 0 ? (long)k.share_max : (long)q * k.simds / 4;
  if (k.share_off || B > cap) return 0;
  const int w = k.share_w ? k.share_w : (4 * B <= 3 * k.simds ? 3 : 2);
  if (has_map)  // a map set: its term on the last aux wavefront; two wavefronts per SIMD, so three per solve up to half a solve per SIMD
    return N > 64 ? 2 : k.share_w ? k.share_w : (2 * B <= k.simds ? 3 : (B <= k.simds ? 2 : 0));
  return w == 3 && (M < 2 || N > 64) ? 2 : w;  // (horizons 65 … 127: two steps per lane, built for two wavefronts)
}

// LDS a solve of the one-wavefront family may take with its obstacle table inside.  32 KiB keeps five solves per CU resident — what a
// batch beyond one solve per SIMD needs; a batch of at most k ≤ 4 solves per CU cannot use that residency, and each of its solves may
// as well have 1/k of the CU's 160 KiB (beyond 64 KiB the launcher raises the kernels' limit): the table of up to ≈ 20 obstacles at two
// solves per CU, ≈ 45 at one, then lies in LDS instead of being streamed from the workspace by every pass, and the shape can take the
// shared-phase-L kernel (tools/share_ab.py, N = 50: M = 12 at B = 256 0.485 → 0.370 ms, M = 8 at B = 1024 0.503 → 0.435 ms).
inline size_t lds_table_budget(const SolveKnobs& kn, int B) {
  if (kn.tab_budget_kb > 0) return (size_t)kn.tab_budget_kb * 1024;  // (CILQR_LDS_TABLE_KB: A/B hook)
  const int cus = kn.simds / 4, k = (B + cus - 1) / cus;
  if (k < 1 || k > 4) return 32 * 1024;
  const size_t share = (160 * 1024) / k - 2048;
  return share < 32 * 1024 ? 32 * 1024 : share;
}

// The plan of one call.  The table of static obstacles lies in LDS while GENERAL kernel + table stay within lds_table_budget (M = 0: an
// empty table fits).  The kernels with further wavefronts per solve are built for the early-exit loop and a table in LDS; where one
// does not apply, cilqr_solve_kernel runs:
//   SPLIT  sampled obstacles, shape as split_shape_wavefronts says, both kernels within the default 64 KiB of LDS;
//   PAIR   CILQR_PAIR_KERNEL, up to one solve per SIMD, no map, both kernels within the default 64 KiB (the experiment was measured
//          and tested on small tables only; slower at every batch size, DESIGN.md §5: not the default);
//   SHARE  static obstacles, N ≤ 127, wavefronts as share_wavefronts says — one fewer, or the one-wavefront kernel, where their partial
//          sums would take the solve past the CU's 160 KiB (beyond 64 KiB the launcher raises both kernels' limit).
inline WavePlan plan_wave(const SolveKnobs& k, const WaveShape& s) {
  const int N = s.N, S = s.path_samples;
  const bool sampled = s.n_samples > 0, early_exit = (s.flags & CILQR_FLAG_FAITHFUL_ITERS) == 0;
  WavePlan p{};
  p.kernel = WavePlan::ONE; p.W = 1;
  p.hinted = !k.hint_off && s.B > k.simds;
  p.tab = sampled ? 2 : one_lds_bytes(N, S, false, table_lds_bytes(N, s.M)) <= lds_table_budget(k, s.B) ? 1 : 0;
  p.shared_table = p.tab == 0 && s.obs_shared;
  const size_t extra = sampled ? sampled_lds_bytes(s.M, s.n_samples) : p.tab == 1 ? table_lds_bytes(N, s.M) : 0;
  p.lds_fast = one_lds_bytes(N, S, early_exit, extra);
  p.lds_general = one_lds_bytes(N, S, false, extra);  // the larger of the two layouts
  p.too_large = p.lds_general > SOLVE_LDS_MAX;
  if (p.too_large || !early_exit || p.tab == 0) return p;
  const auto with = [&](WavePlan::Kernel kernel, int W, size_t lds_fast, size_t limit) {  // that kernel first, if W > 1 and both kernels stay within `limit`; else p
    WavePlan m = p;
    m.kernel = kernel; m.W = W; m.lds_fast = lds_fast; m.long_form = kernel == WavePlan::SHARE && N > dev::WAVE;
    return W > 1 && lds_fast <= limit && p.lds_general <= limit ? m : p;
  };
  if (sampled) {
    const int W = split_shape_wavefronts(k, s.B, N, s.M);
    return with(WavePlan::SPLIT, W, split_lds_bytes(N, S, W, s.has_map, extra), SOLVE_LDS_DEFAULT);
  }
  if (k.pair_on && s.B <= k.simds) return with(WavePlan::PAIR, s.has_map ? 1 : 2, pair_lds_bytes(N, S, extra), SOLVE_LDS_DEFAULT);
  // (every further wavefront adds 5N partial sums: where three no longer fit the CU beside a large table, two may — and else one)
  int W = N < 2 * dev::WAVE ? share_wavefronts(k, s.B, N, s.M, s.has_map) : 1;
  while (W > 1 && share_lds_bytes(N, S, W, s.has_map, extra) > SOLVE_LDS_MAX) --W;
  return with(WavePlan::SHARE, W, share_lds_bytes(N, S, W, s.has_map, extra), SOLVE_LDS_MAX);
}

// cilqr_solve_wavefronts (include/cilqr.h): the wavefronts of the share kernel where an ordinary call of this shape (no flags, the
// handle's map) runs on it, else 1 — also 1 under CILQR_PAIR_KERNEL, at every batch size.
inline int query_wavefronts(const SolveKnobs& k, int B, int N, int M, int path_samples, bool has_map) {
  const WavePlan p = plan_wave(k, {B, N, M, 0, path_samples, 0, has_map, false});
  return !k.pair_on && plan_group_lanes(k, B, N, M) == 64 && p.kernel == WavePlan::SHARE ? p.W : 1;
}

}  // namespace cilqr
