// costmap_polygons.hip — obstacle bounding boxes rasterised into a costmap layer on gfx950 (MI355X).
//
// Reference: LocalCostmap::bondingBoxHandle (M/src/local_costmap.cpp:860-922): a grid_map::PolygonIterator per tracked
// vehicle writes 100 into the freshly cleared (all-NaN) bounding_box_map.  The iterator visits the cells of the polygon's
// bounding submap whose centre passes Polygon::isInside (G/grid_map_core/src/Polygon.cpp:32-44); here every cell of the
// layer is decided by that same test (costmap_polygons.hpp) on the centre the warp kernels compute, fp64 with contraction
// OFF and IEEE division, so a centre that sits on an edge falls to the same side as in the reference.
// Layout as warp_batch_kernel's: float32 column-major, lanes along i with four consecutive rows each, one 16-byte store per
// lane and column where the rows come in fours.  A workgroup owns a 256(i) x 8(j) tile; wave w has columns w and w + 4.
#include "cilqr_internal.h"
#include "costmap_polygons.hpp"

namespace cilqr {

namespace {

constexpr int NTHREADS = 256;
constexpr int RT_I = 256, RT_J = 8;

// CLEAR: every cell is written (value inside a polygon, NaN elsewhere); otherwise only the cells inside a polygon are.
template <bool CLEAR>
__global__ __launch_bounds__(NTHREADS) void rasterize_kernel(const double* __restrict__ table, int n_polygons, int V, cilqr_map_geom g, float value,
                                                             float* __restrict__ layer, int tiles_i) {
#pragma clang fp contract(off)
  const int ti = blockIdx.x % tiles_i, tj = blockIdx.x / tiles_i;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = ti * RT_I + 4 * lane;
  const int rows = g.rows, cols = g.cols;
  const double off_x = 0.5 * g.len_x - 0.5 * g.res, off_y = 0.5 * g.len_y - 0.5 * g.res;
  double px[4], py[RT_J / 4];
#pragma unroll
  for (int k = 0; k < 4; ++k) px[k] = (g.pos_x + off_x) + g.res * (double)(-(i0 + k));
#pragma unroll
  for (int jj = 0; jj < RT_J / 4; ++jj) py[jj] = (g.pos_y + off_y) + g.res * (double)(-(tj * RT_J + wave + 4 * jj));
  unsigned hit[RT_J / 4];
  polygons_cover<4, RT_J / 4>(table, n_polygons, V, ti * RT_I, ti * RT_I + RT_I - 1, tj * RT_J, tj * RT_J + RT_J - 1, px, py, hit);

  const float nan = __builtin_nanf("");
  const bool fours = (rows & 3) == 0;  // then a lane's rows are all inside or all outside, and every column starts 16-byte aligned
#pragma unroll
  for (int jj = 0; jj < RT_J / 4; ++jj) {
    const int j = tj * RT_J + wave + 4 * jj;
    if (j >= cols || i0 >= rows) break;
    const size_t lin = (size_t)j * rows + i0;
    const unsigned h = hit[jj];
    if (CLEAR && fours) {
      *reinterpret_cast<float4*>(layer + lin) = make_float4((h & 1) ? value : nan, (h & 2) ? value : nan, (h & 4) ? value : nan, (h & 8) ? value : nan);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i0 + k >= rows) break;
        if ((h >> k) & 1) layer[lin + k] = value;
        else if (CLEAR) layer[lin + k] = nan;
      }
    }
  }
}

}  // namespace

hipError_t launch_rasterize_polygons(const PolygonTable& t, const cilqr_map_geom& g, float value, bool clear, float* layer, hipStream_t stream) {
  if (!clear && t.n == 0) return hipSuccess;
  const int tiles_i = (g.rows + RT_I - 1) / RT_I, tiles_j = (g.cols + RT_J - 1) / RT_J;
  if (clear) hipLaunchKernelGGL(rasterize_kernel<true>, dim3(tiles_i * tiles_j), dim3(NTHREADS), 0, stream, t.table, t.n, t.V, g, value, layer, tiles_i);
  else hipLaunchKernelGGL(rasterize_kernel<false>, dim3(tiles_i * tiles_j), dim3(NTHREADS), 0, stream, t.table, t.n, t.V, g, value, layer, tiles_i);
  return hipGetLastError();
}

}  // namespace cilqr
