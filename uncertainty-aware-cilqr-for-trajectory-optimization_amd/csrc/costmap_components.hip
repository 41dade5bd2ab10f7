// costmap_components.hip — obstacles from the map (cilqr_map_obstacles*, include/cilqr.h): the connected components of the linked
// cells of L distance fields, their integer moments, and the principal-axis box of each as an obstacle row.
//
// A cell is LINKED where d2 <= gap2 (d2 the field of cilqr_map_distance, INT32_MAX never) and a SEED where d2 == 0.  The label of a
// linked cell is the lowest linear index i + j*rows among the linked cells of its component; union and find are those of
// costmap_components.hpp, every loop bounded by rows·cols.  Seven launches behind one clear of n_out:
//   tiles    one workgroup per 64 x 16 tile: lane along i (consecutive words of the column-major field), four cells a lane;
//            union-find over the tile in LDS; the tile's roots leave as global indices.  Clears `work`.
//   seams    lane = cell: a linked cell unites with its lower neighbours that lie in ANOTHER tile, by atomic minima in label_out.
//   flatten  lane = cell: label = find; a seed adds 1 to work[label]: the seeds of each component, counted at its root.
//   rank     one workgroup per layer walks the cells in index order, 1024 at a time: a root whose count reaches min_cells gets the
//            next slot (ballot prefix), the first K of them a row of comp, initialised as raw 64-bit integers; work[root] = slot.
//   moments  lane = linked cell: counts, index sums and index extremes go into the slot's row by 64-bit integer atomics — once per
//            wavefront where the wavefront's linked cells share a slot, which is the rule inside a blob.
//   extents  one workgroup per slot: the axis from the moments, then the extremes of p and q over the seeds of the slot's index
//            window (minima and maxima: no order matters); one lane forms the box, converts the row to doubles in place and writes the
//            box at the slot's place; a box above max_size leaves LABEL = -1.
//   finish   one workgroup per layer: the kept rows move down in order (a row only ever moves to a lower place: read, barrier,
//            write), the rest become filler rows, n_out is completed.
// Integer sums, minima and maxima only: a layer's bits depend on that layer alone.  No scratch memory, nothing allocated.
// An overrun of a loop bound leaves n_out[l][2] = -1 from the launch that saw it; `finish` then writes -1 into all of n_out[l] and
// filler into every row.
#include <limits.h>

#include "cilqr_internal.h"
#include "costmap_components.hpp"

namespace cilqr {

namespace {

constexpr int F = CILQR_MAP_OBSTACLE_FIELDS;
constexpr unsigned long long INDEX_NONE = 1ull << 20;  // above every index along a side

template <int SCOPE>
struct CcDeviceMem {
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE); }
};
using LdsMem = CcDeviceMem<__HIP_MEMORY_SCOPE_WORKGROUP>;
using GlobalMem = CcDeviceMem<__HIP_MEMORY_SCOPE_AGENT>;

__device__ __forceinline__ bool is_linked(int d2, int gap2) { return d2 != INT_MAX && d2 <= gap2; }
__device__ __forceinline__ int neighbours(uint32_t flags) { return (flags & CILQR_MAP_OBSTACLES_FOUR) ? 2 : CC_NEIGHBOURS; }
__device__ __forceinline__ void raise_overrun(const MapObstaclesArgs& a, int l) { atomicMin(a.n_out + 4 * l + 2, -1); }

// the lane's place among the lanes of the workgroup whose flag is set, and their number; `totals` holds one int per wavefront.
// Two barriers: the caller may reuse `totals` right away.
__device__ __forceinline__ int block_rank(bool flag, int* totals, int* total) {
  const unsigned long long votes = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
  if (lane == 0) totals[wave] = __popcll(votes);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < waves; ++w) {
    const int n = totals[w];
    before += w < wave ? n : 0;
    all += n;
  }
  __syncthreads();
  *total = all;
  return before + __popcll(votes & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// grid L·ceil(rows/64)·ceil(cols/16), layer slowest
__global__ __launch_bounds__(MAP_OBSTACLES_THREADS) void cilqr_map_obstacles_tiles_kernel(MapObstaclesArgs a) {
  __shared__ int lab[CC_TILE_I * CC_TILE_J];
  constexpr int PER_LANE = CC_TILE_I * CC_TILE_J / MAP_OBSTACLES_THREADS, STEP_J = MAP_OBSTACLES_THREADS / CC_TILE_I;
  const int rows = a.rows, cols = a.cols;
  const int ti_n = (rows + CC_TILE_I - 1) / CC_TILE_I, tj_n = (cols + CC_TILE_J - 1) / CC_TILE_J;
  const int l = blockIdx.x / (ti_n * tj_n), t = blockIdx.x - l * (ti_n * tj_n);
  const int i0 = (t % ti_n) * CC_TILE_I, j0 = (t / ti_n) * CC_TILE_J;
  const size_t base = (size_t)l * ((size_t)rows * cols);
  const int li = threadIdx.x % CC_TILE_I, lj0 = threadIdx.x / CC_TILE_I, i = i0 + li;
  unsigned linked = 0;
  for (int k = 0; k < PER_LANE; ++k) {
    const int lj = lj0 + k * STEP_J, j = j0 + lj;
    bool on = false;
    if (i < rows && j < cols) {
      const size_t at = base + (size_t)j * rows + i;
      on = is_linked(a.d2[at], a.gap2);
      a.work[at] = 0;
    }
    lab[li + lj * CC_TILE_I] = on ? li + lj * CC_TILE_I : -1;
    linked |= on ? 1u << k : 0u;
  }
  __syncthreads();
  int overrun = 0;
  const int nk = neighbours(a.flags);
  for (int k = 0; k < PER_LANE; ++k) {
    if (!(linked >> k & 1u)) continue;
    const int lj = lj0 + k * STEP_J, loc = li + lj * CC_TILE_I;
    for (int n = 0; n < nk; ++n) {
      int di, dj;
      cc_neighbour(n, &di, &dj);
      const int ni = li + di, nj = lj + dj;
      if (ni < 0 || ni >= CC_TILE_I || nj < 0) continue;  // (in another tile: the seams)
      const int other = ni + nj * CC_TILE_I;
      if (LdsMem::load(lab + other) >= 0) cc_union<LdsMem>(lab, loc, other, CC_TILE_I * CC_TILE_J, &overrun);
    }
  }
  __syncthreads();
  for (int k = 0; k < PER_LANE; ++k) {
    const int lj = lj0 + k * STEP_J, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    int label = -1;
    if (linked >> k & 1u) {
      const int r = cc_find<LdsMem>(lab, li + lj * CC_TILE_I, CC_TILE_I * CC_TILE_J, &overrun);
      label = (i0 + r % CC_TILE_I) + (j0 + r / CC_TILE_I) * rows;
    }
    a.label_out[base + (size_t)j * rows + i] = label;
  }
  if (overrun) raise_overrun(a, l);
}

// grid L·ceil(cells / MAP_OBSTACLES_THREADS), layer slowest (the two launches below too)
__global__ __launch_bounds__(MAP_OBSTACLES_THREADS) void cilqr_map_obstacles_seams_kernel(MapObstaclesArgs a) {
  const int rows = a.rows, cols = a.cols, cells = rows * cols;
  const int chunks = (cells + MAP_OBSTACLES_THREADS - 1) / MAP_OBSTACLES_THREADS;
  const int l = blockIdx.x / chunks, c = (blockIdx.x - l * chunks) * MAP_OBSTACLES_THREADS + threadIdx.x;
  if (c >= cells) return;
  const int i = c % rows, j = c / rows;
  const int ei = i % CC_TILE_I, ej = j % CC_TILE_J;
  if (ei != 0 && ei != CC_TILE_I - 1 && ej != 0) return;  // no lower neighbour of this cell lies in another tile
  int* P = a.label_out + (size_t)l * cells;
  if (GlobalMem::load(P + c) < 0) return;
  int overrun = 0;
  const int nk = neighbours(a.flags);
  for (int n = 0; n < nk; ++n) {
    int di, dj;
    cc_neighbour(n, &di, &dj);
    const int ni = i + di, nj = j + dj;
    if (ni < 0 || ni >= rows || nj < 0) continue;
    if (ni / CC_TILE_I == i / CC_TILE_I && nj / CC_TILE_J == j / CC_TILE_J) continue;  // (united in LDS already)
    const int other = ni + nj * rows;
    if (GlobalMem::load(P + other) >= 0) cc_union<GlobalMem>(P, c, other, cells, &overrun);
  }
  if (overrun) raise_overrun(a, l);
}

__global__ __launch_bounds__(MAP_OBSTACLES_THREADS) void cilqr_map_obstacles_flatten_kernel(MapObstaclesArgs a) {
  const int cells = a.rows * a.cols;
  const int chunks = (cells + MAP_OBSTACLES_THREADS - 1) / MAP_OBSTACLES_THREADS;
  const int l = blockIdx.x / chunks, c = (blockIdx.x - l * chunks) * MAP_OBSTACLES_THREADS + threadIdx.x;
  if (c >= cells) return;
  const size_t base = (size_t)l * cells;
  int* P = a.label_out + base;
  if (GlobalMem::load(P + c) < 0) return;
  int overrun = 0;
  const int r = cc_find<GlobalMem>(P, c, cells, &overrun);
  if (r != c) __hip_atomic_store(P + c, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a root keeps itself: others walk through it)
  if (a.d2[base + c] == 0) atomicAdd(a.work + base + r, 1);
  if (overrun) raise_overrun(a, l);
}

// grid L; MAP_OBSTACLES_RANK_THREADS lanes
__global__ __launch_bounds__(MAP_OBSTACLES_RANK_THREADS) void cilqr_map_obstacles_rank_kernel(MapObstaclesArgs a) {
  __shared__ int totals[MAP_OBSTACLES_RANK_THREADS / 64];
  const int cells = a.rows * a.cols, l = blockIdx.x;
  const size_t base = (size_t)l * cells;
  const int* P = a.label_out + base;
  int* work = a.work + base;
  int passed = 0, found = 0, seeds = 0;
  for (int c0 = 0; c0 < cells; c0 += MAP_OBSTACLES_RANK_THREADS) {
    const int c = c0 + (int)threadIdx.x;
    const bool root = c < cells && P[c] == c;
    const int count = root ? work[c] : 0;
    const bool pass = root && count >= a.min_cells;
    found += root ? 1 : 0;
    seeds += count;
    int total;
    const int rank = passed + block_rank(pass, totals, &total);
    passed += total;
    if (root) {
      const int slot = pass && rank < a.K ? rank : -1;
      work[c] = slot;
      if (slot >= 0) {
        unsigned long long* raw = (unsigned long long*)(a.comp + ((size_t)l * a.K + slot) * F);
        for (int f = 0; f < F; ++f) raw[f] = 0ull;
        raw[CILQR_MO_LABEL] = (unsigned long long)c;
        raw[CILQR_MO_CELLS] = (unsigned long long)count;
        raw[CILQR_MO_I_MIN] = INDEX_NONE;
        raw[CILQR_MO_J_MIN] = INDEX_NONE;
      }
    }
  }
  found = wave_sum(found);
  seeds = wave_sum(seeds);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(a.n_out + 4 * l + 0, found);
    atomicAdd(a.n_out + 4 * l + 3, seeds);
  }
  if (threadIdx.x == 0) a.n_out[4 * l + 1] = passed;
}

__global__ __launch_bounds__(MAP_OBSTACLES_THREADS) void cilqr_map_obstacles_moments_kernel(MapObstaclesArgs a) {
  const int rows = a.rows, cells = rows * a.cols;
  const int chunks = (cells + MAP_OBSTACLES_THREADS - 1) / MAP_OBSTACLES_THREADS;
  const int l = blockIdx.x / chunks, c = (blockIdx.x - l * chunks) * MAP_OBSTACLES_THREADS + threadIdx.x;
  const size_t base = (size_t)l * cells;
  int slot = -1;
  bool seed = false;
  if (c < cells) {
    const int label = a.label_out[base + c];
    if (label >= 0) slot = a.work[base + label];
    if (slot >= a.K || a.n_out[4 * l + 2] < 0) slot = -1;  // (only after an overrun can a label be no root: nothing is added then)
    seed = slot >= 0 && a.d2[base + c] == 0;
  }
  const unsigned long long live = __ballot(slot >= 0);
  if (live == 0ull) return;  // (the whole wavefront)
  const int first = __shfl(slot, __ffsll((long long)live) - 1);
  const bool shared = __ballot(slot >= 0 && slot != first) == 0ull;
  const int i = c % rows, j = c / rows;  // (both below 1024: every product below fits an int, and so does a wavefront's sum)
  int n = slot >= 0 ? 1 : 0;
  int si = seed ? i : 0, sj = seed ? j : 0, sii = seed ? i * i : 0, sij = seed ? i * j : 0, sjj = seed ? j * j : 0;
  int i_lo = seed ? i : (int)INDEX_NONE, i_hi = seed ? i : 0, j_lo = seed ? j : (int)INDEX_NONE, j_hi = seed ? j : 0;
  bool writer = slot >= 0;
  if (shared) {
    n = wave_sum(n); si = wave_sum(si); sj = wave_sum(sj); sii = wave_sum(sii); sij = wave_sum(sij); sjj = wave_sum(sjj);
    i_lo = wave_min(i_lo); i_hi = wave_max(i_hi); j_lo = wave_min(j_lo); j_hi = wave_max(j_hi);
    slot = first;
    writer = (threadIdx.x & 63) == 0;
  }
  if (!writer) return;
  unsigned long long* raw = (unsigned long long*)(a.comp + ((size_t)l * a.K + slot) * F);
  atomicAdd(raw + CILQR_MO_LINKED, (unsigned long long)n);
  if (i_lo > i_hi) return;  // no seed among them
  atomicMin(raw + CILQR_MO_I_MIN, (unsigned long long)i_lo);
  atomicMax(raw + CILQR_MO_I_MAX, (unsigned long long)i_hi);
  atomicMin(raw + CILQR_MO_J_MIN, (unsigned long long)j_lo);
  atomicMax(raw + CILQR_MO_J_MAX, (unsigned long long)j_hi);
  atomicAdd(raw + CILQR_MO_SUM_I, (unsigned long long)si);
  atomicAdd(raw + CILQR_MO_SUM_J, (unsigned long long)sj);
  atomicAdd(raw + CILQR_MO_SUM_II, (unsigned long long)sii);
  atomicAdd(raw + CILQR_MO_SUM_IJ, (unsigned long long)sij);
  atomicAdd(raw + CILQR_MO_SUM_JJ, (unsigned long long)sjj);
}

__device__ __forceinline__ double wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// grid L·K, layer slowest
__global__ __launch_bounds__(MAP_OBSTACLES_THREADS) void cilqr_map_obstacles_extents_kernel(MapObstaclesArgs a) {
#pragma clang fp contract(off)  // the header's formulas, evaluated as C evaluates them
  __shared__ double part[4][MAP_OBSTACLES_THREADS / 64];
  const int l = blockIdx.x / a.K, s = blockIdx.x - l * a.K;
  if (a.n_out[4 * l + 2] < 0 || s >= min(a.n_out[4 * l + 1], a.K)) return;  // (the whole workgroup)
  const int rows = a.rows;
  const size_t base = (size_t)l * ((size_t)rows * a.cols);
  double* row = a.comp + ((size_t)l * a.K + s) * F;
  long long v[F];
  for (int f = 0; f < F; ++f) v[f] = (long long)((const unsigned long long*)row)[f];
  const long long c = v[CILQR_MO_CELLS], Si = v[CILQR_MO_SUM_I], Sj = v[CILQR_MO_SUM_J];
  const long long ma = c * v[CILQR_MO_SUM_II] - Si * Si, mb = c * v[CILQR_MO_SUM_IJ] - Si * Sj, md = c * v[CILQR_MO_SUM_JJ] - Sj * Sj;
  const double phi = 0.5 * atan2(2.0 * (double)mb, (double)ma - (double)md);
  double so, co;
  sincos(phi, &so, &co);
  const double mi = (double)Si / (double)c, mj = (double)Sj / (double)c;
  const int label = (int)v[CILQR_MO_LABEL];
  const int i_lo = (int)v[CILQR_MO_I_MIN], j_lo = (int)v[CILQR_MO_J_MIN];
  const int wi = (int)v[CILQR_MO_I_MAX] - i_lo + 1, wj = (int)v[CILQR_MO_J_MAX] - j_lo + 1;  // (>= 1: a slot has a seed)
  double p_lo = __builtin_huge_val(), p_hi = -__builtin_huge_val(), q_lo = __builtin_huge_val(), q_hi = -__builtin_huge_val();
  for (int w = threadIdx.x; w < wi * wj; w += MAP_OBSTACLES_THREADS) {
    const int i = i_lo + w % wi, j = j_lo + w / wi;  // (inside the layer: the window is made of seeds' indices)
    const size_t at = base + (size_t)j * rows + i;
    if (a.d2[at] != 0 || a.label_out[at] != label) continue;
    const double di = (double)i - mi, dj = (double)j - mj;
    const double p = di * co + dj * so, q = dj * co - di * so;
    p_lo = fmin(p_lo, p); p_hi = fmax(p_hi, p); q_lo = fmin(q_lo, q); q_hi = fmax(q_hi, q);
  }
  p_lo = wave_min(p_lo); p_hi = wave_max(p_hi); q_lo = wave_min(q_lo); q_hi = wave_max(q_hi);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[0][wave] = p_lo; part[1][wave] = p_hi; part[2][wave] = q_lo; part[3][wave] = q_hi; }
  __syncthreads();  // (every lane has read the raw row by now, too)
  if (threadIdx.x != 0) return;
  for (int w = 0; w < MAP_OBSTACLES_THREADS / 64; ++w) {
    p_lo = fmin(p_lo, part[0][w]); p_hi = fmax(p_hi, part[1][w]); q_lo = fmin(q_lo, part[2][w]); q_hi = fmax(q_hi, part[3][w]);
  }
  const double h = 0.5 * (fabs(co) + fabs(so));
  const double p0 = p_lo - h, p1 = p_hi + h, q0 = q_lo - h, q1 = q_hi + h;
  const double pc = 0.5 * (p0 + p1), qc = 0.5 * (q0 + q1);
  const double ci = mi + pc * co - qc * so, cj = mj + pc * so + qc * co;
  const double mx = a.x_first - ci * a.res, my = a.y_first - cj * a.res;
  double px = 0.0, py = 0.0, th = 0.0;
  if (a.pose) {
    const double* ps = a.pose + (size_t)l * a.pose_stride;
    px = ps[0]; py = ps[1]; th = ps[2];
  }
  double sn, cs;
  sincos(th, &sn, &cs);
  const double x = px + (cs * mx - sn * my), y = py + (sn * mx + cs * my), yaw = phi + th;
  const double size_x = (p1 - p0) * a.res + 2.0 * a.pad, size_y = (q1 - q0) * a.res + 2.0 * a.pad;
  const bool drop = fmax(size_x, size_y) > a.max_size;
  for (int f = 0; f < F; ++f) row[f] = (double)v[f];
  row[CILQR_MO_FILL] = (double)c / ((p1 - p0) * (q1 - q0));
  if (drop) row[CILQR_MO_LABEL] = -1.0;
  const size_t at = (size_t)l * a.K + s;
  if (a.boxes) {
    double* b = a.boxes + at * 5;
    b[0] = x; b[1] = y; b[2] = yaw; b[3] = size_x; b[4] = size_y;
  }
  if (a.pose_out) {
    double* o = a.pose_out + at * 4;
    o[0] = x; o[1] = y; o[2] = 0.0; o[3] = yaw;
  }
  if (a.dim_out) {
    double* o = a.dim_out + at * 2;
    o[0] = size_x; o[1] = size_y;
  }
}

// grid L
__global__ __launch_bounds__(MAP_OBSTACLES_THREADS) void cilqr_map_obstacles_finish_kernel(MapObstaclesArgs a) {
  __shared__ int totals[MAP_OBSTACLES_THREADS / 64];
  const int l = blockIdx.x, K = a.K;
  const bool overrun = a.n_out[4 * l + 2] < 0;
  const int slots = overrun ? 0 : min(a.n_out[4 * l + 1], K);
  double* comp = a.comp + (size_t)l * K * F;
  double* boxes = a.boxes ? a.boxes + (size_t)l * K * 5 : nullptr;
  double* pose_out = a.pose_out ? a.pose_out + (size_t)l * K * 4 : nullptr;
  double* dim_out = a.dim_out ? a.dim_out + (size_t)l * K * 2 : nullptr;
  int written = 0;
  for (int s0 = 0; s0 < slots; s0 += MAP_OBSTACLES_THREADS) {
    const int s = s0 + (int)threadIdx.x;
    const bool keep = s < slots && comp[(size_t)s * F + CILQR_MO_LABEL] >= 0.0;
    double r[F], b[5], p[4], d[2];
    if (keep) {
      for (int f = 0; f < F; ++f) r[f] = comp[(size_t)s * F + f];
      if (boxes) for (int f = 0; f < 5; ++f) b[f] = boxes[(size_t)s * 5 + f];
      if (pose_out) for (int f = 0; f < 4; ++f) p[f] = pose_out[(size_t)s * 4 + f];
      if (dim_out) for (int f = 0; f < 2; ++f) d[f] = dim_out[(size_t)s * 2 + f];
    }
    int total;
    const int to = written + block_rank(keep, totals, &total);  // (its barriers stand between this chunk's reads and its writes)
    written += total;
    if (keep) {
      for (int f = 0; f < F; ++f) comp[(size_t)to * F + f] = r[f];
      if (boxes) for (int f = 0; f < 5; ++f) boxes[(size_t)to * 5 + f] = b[f];
      if (pose_out) for (int f = 0; f < 4; ++f) pose_out[(size_t)to * 4 + f] = p[f];
      if (dim_out) for (int f = 0; f < 2; ++f) dim_out[(size_t)to * 2 + f] = d[f];
    }
    __syncthreads();  // the next chunk reads rows above every place written so far, and only after this
  }
  const double far = CILQR_MAP_OBSTACLES_FAR;
  for (int s = written + (int)threadIdx.x; s < K; s += MAP_OBSTACLES_THREADS) {
    for (int f = 0; f < F; ++f) comp[(size_t)s * F + f] = -1.0;
    if (boxes) { double* b = boxes + (size_t)s * 5; b[0] = far; b[1] = far; b[2] = 0.0; b[3] = 0.0; b[4] = 0.0; }
    if (pose_out) { double* p = pose_out + (size_t)s * 4; p[0] = far; p[1] = far; p[2] = 0.0; p[3] = 0.0; }
    if (dim_out) { double* d = dim_out + (size_t)s * 2; d[0] = 0.0; d[1] = 0.0; }
  }
  if (threadIdx.x == 0) {
    a.n_out[4 * l + 2] = written;
    if (overrun) for (int f = 0; f < 4; ++f) a.n_out[4 * l + f] = -1;
  }
}

}  // namespace

hipError_t launch_map_obstacles(const MapObstaclesArgs& a, hipStream_t stream) {
  if (a.L <= 0) return hipSuccess;
  // (the host checked that every grid stays below 2^31 workgroups)
  const unsigned L = (unsigned)a.L, cells = (unsigned)a.rows * (unsigned)a.cols;
  const unsigned tiles = (unsigned)((a.rows + CC_TILE_I - 1) / CC_TILE_I) * (unsigned)((a.cols + CC_TILE_J - 1) / CC_TILE_J);
  const unsigned chunks = (cells + MAP_OBSTACLES_THREADS - 1) / MAP_OBSTACLES_THREADS;
  hipError_t e = hipMemsetAsync(a.n_out, 0, (size_t)a.L * 4 * sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
#define CILQR_MO_LAUNCH(kernel, grid, threads)                                  \
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, stream, a);          \
  e = hipGetLastError();                                                        \
  if (e != hipSuccess) return e
  CILQR_MO_LAUNCH(cilqr_map_obstacles_tiles_kernel, tiles * L, MAP_OBSTACLES_THREADS);
  CILQR_MO_LAUNCH(cilqr_map_obstacles_seams_kernel, chunks * L, MAP_OBSTACLES_THREADS);
  CILQR_MO_LAUNCH(cilqr_map_obstacles_flatten_kernel, chunks * L, MAP_OBSTACLES_THREADS);
  CILQR_MO_LAUNCH(cilqr_map_obstacles_rank_kernel, L, MAP_OBSTACLES_RANK_THREADS);
  CILQR_MO_LAUNCH(cilqr_map_obstacles_moments_kernel, chunks * L, MAP_OBSTACLES_THREADS);
  CILQR_MO_LAUNCH(cilqr_map_obstacles_extents_kernel, (unsigned)a.K * L, MAP_OBSTACLES_THREADS);
  CILQR_MO_LAUNCH(cilqr_map_obstacles_finish_kernel, L, MAP_OBSTACLES_THREADS);
#undef CILQR_MO_LAUNCH
  return hipSuccess;
}

}  // namespace cilqr
