// costmap_distance.hip — distance to the occupied cells of a layer (cilqr_map_distance*, cilqr_inflate_map*, include/cilqr.h): the
// exact squared Euclidean distance transform of L layers, in cells, and a layer inflated from that field for the solve to read.
//
// A SEED is a cell whose value is finite and > occ_threshold (strict), optionally a NaN cell too, optionally the complement of
// that set.  d2(i, j) = min over the seeds (i', j') of (i - i')² + (j - j')²: the minimum separates into a minimum along the
// row and one along the column, so two launches give it exactly, in integers:
//   rows     lane = row index i of layer l: consecutive lanes read consecutive floats of the column-major layer.  The lane walks
//            j = 0 ... cols - 1 carrying the distance to the last seed of its row, writes it, then walks back and keeps the smaller.
//            A row without a seed holds DIST_NONE = 2^15 everywhere: its square, 2^30, is above every real d2 (<= 2·8191²) and
//            its sum with any (i - i')² still fits an int32.
//   columns  one workgroup per (layer, column j): the column's `rows` contiguous values go to LDS squared, G[i].  Lane = i (strided)
//            searches outward, best = min over delta = 0, 1, ... of min(G[i - delta], G[i + delta]) + delta², and stops once
//            delta² >= best: no farther row can give less.  The result replaces the column in place; 2^30 or more means no seed
//            anywhere in the layer: INT32_MAX.  Neighbouring lanes read neighbouring LDS words: no bank conflict.
// Integer minima only: a layer's bits depend on that layer alone, whatever L is.  No atomics, no scratch memory, nothing allocated;
// LDS is 4·rows bytes (rows <= 8192: 32 KiB).
//   inflate  lane = cell: d = res·sqrt(d2) in doubles, the ramp between `inscribed` and `radius`, max with the cell.
#include <limits.h>

#include "cilqr_internal.h"

namespace cilqr {

namespace {

constexpr int DIST_NONE = 1 << 15;       // row distance of a row without a seed
constexpr int DIST2_NONE = 1 << 30;      // its square: "no seed" once the columns are merged

__device__ __forceinline__ bool is_seed(float v, double threshold, uint32_t flags) {
  const bool known = v == v;
  bool seed = known && fabsf(v) <= 3.4028234663852886e38f && (double)v > threshold;
  if ((flags & CILQR_MAP_DISTANCE_UNKNOWN_SEEDS) && !known) seed = true;
  return (flags & CILQR_MAP_DISTANCE_TO_FREE) ? !seed : seed;
}

// grid L·ceil(rows / MAP_DISTANCE_THREADS), layer slowest
__global__ __launch_bounds__(MAP_DISTANCE_THREADS) void cilqr_map_distance_rows_kernel(MapDistanceArgs a) {
  const int rows = a.rows, cols = a.cols;
  const int tiles = (rows + MAP_DISTANCE_THREADS - 1) / MAP_DISTANCE_THREADS;
  const int l = blockIdx.x / tiles, i = (blockIdx.x - l * tiles) * MAP_DISTANCE_THREADS + threadIdx.x;
  if (i >= rows) return;
  const float* in = a.layer + (size_t)l * (size_t)a.layer_stride + i;
  int32_t* out = a.d2_out + (size_t)l * ((size_t)rows * cols) + i;
  int run = DIST_NONE;
  for (int j = 0; j < cols; ++j) {
    const size_t at = (size_t)j * rows;
    run = is_seed(in[at], a.occ_threshold, a.flags) ? 0 : min(run + 1, DIST_NONE);
    out[at] = run;
  }
  // (run: the last column's distance to a seed on its left, which is what the walk back starts from)
  for (int j = cols - 2; j >= 0; --j) {
    const size_t at = (size_t)j * rows;
    const int left = out[at];  // (written by this lane above)
    run = min(left, min(run + 1, DIST_NONE));
    out[at] = run;
  }
}

// grid L·cols, layer slowest; dynamic LDS: rows int32
__global__ __launch_bounds__(MAP_DISTANCE_THREADS) void cilqr_map_distance_cols_kernel(MapDistanceArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t dist_lds[];
  const int rows = a.rows, cols = a.cols;
  const int tid = threadIdx.x, l = blockIdx.x / cols, j = blockIdx.x - l * cols;
  const size_t at = (size_t)l * ((size_t)rows * cols) + (size_t)j * rows;
  int32_t* col = a.d2_out + at;
  for (int i = tid; i < rows; i += MAP_DISTANCE_THREADS) {
    const int g = col[i];
    dist_lds[i] = g * g;
  }
  __syncthreads();
  const double res = a.res;
  for (int i = tid; i < rows; i += MAP_DISTANCE_THREADS) {
    int best = dist_lds[i];
    for (int d = 1; d < rows && d * d < best; ++d) {  // (d <= 8191: d·d fits; best <= 2^30, so best + d·d does too)
      const int lo = i - d >= 0 ? dist_lds[i - d] : DIST2_NONE, hi = i + d < rows ? dist_lds[i + d] : DIST2_NONE;
      best = min(best, min(lo, hi) + d * d);
    }
    const bool none = best >= DIST2_NONE;
    col[i] = none ? INT_MAX : best;
    if (a.dist_out) a.dist_out[at + i] = none ? __builtin_huge_valf() : (float)(res * sqrt((double)best));
  }
}

// grid L·ceil(cells / MAP_DISTANCE_THREADS), layer slowest
__global__ __launch_bounds__(MAP_DISTANCE_THREADS) void cilqr_inflate_map_kernel(InflateMapArgs a) {
#pragma clang fp contract(off)  // the header's formula, evaluated as C evaluates it
  const size_t cells = (size_t)a.rows * a.cols;
  const unsigned tiles = (unsigned)((cells + MAP_DISTANCE_THREADS - 1) / MAP_DISTANCE_THREADS);
  const int l = blockIdx.x / tiles;
  const size_t c = (size_t)(blockIdx.x - l * tiles) * MAP_DISTANCE_THREADS + threadIdx.x;
  if (c >= cells) return;
  const int d2 = a.d2[(size_t)l * cells + c];
  const float o = a.layer[(size_t)l * (size_t)a.layer_stride + c];
  const double d = a.res * sqrt((double)d2);
  double v;
  if (d2 == INT_MAX) v = 0.0;
  else if (d <= a.inscribed) v = a.peak;
  else if (d >= a.radius) v = 0.0;
  else v = a.peak * (a.radius - d) / (a.radius - a.inscribed);
  const float f = (float)v;
  float r;
  if (o == o) r = o > f ? o : f;
  else r = v > 0.0 ? f : o;  // unknown stays unknown where nothing reaches it
  a.layer_out[(size_t)l * cells + c] = r;
}

}  // namespace

hipError_t launch_map_distance(const MapDistanceArgs& a, hipStream_t stream) {
  if (a.L <= 0) return hipSuccess;
  // (the host checked that both grids stay below 2^31 workgroups)
  const unsigned tiles = (unsigned)((a.rows + MAP_DISTANCE_THREADS - 1) / MAP_DISTANCE_THREADS);
  hipLaunchKernelGGL(cilqr_map_distance_rows_kernel, dim3(tiles * (unsigned)a.L), dim3(MAP_DISTANCE_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_map_distance_cols_kernel, dim3((unsigned)a.cols * (unsigned)a.L), dim3(MAP_DISTANCE_THREADS),
                     (size_t)a.rows * sizeof(int32_t), stream, a);
  return hipGetLastError();
}

hipError_t launch_inflate_map(const InflateMapArgs& a, hipStream_t stream) {
  if (a.L <= 0) return hipSuccess;
  const size_t cells = (size_t)a.rows * a.cols;
  const unsigned tiles = (unsigned)((cells + MAP_DISTANCE_THREADS - 1) / MAP_DISTANCE_THREADS);
  hipLaunchKernelGGL(cilqr_inflate_map_kernel, dim3(tiles * (unsigned)a.L), dim3(MAP_DISTANCE_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
