// costmap_polygons.hpp — the point-in-polygon test of the obstacle bounding boxes, shared by the rasteriser
// (costmap_polygons.hip) and the warp kernels' polygon override (costmap_warp.hip).
//
// Reference: Polygon::isInside (G/grid_map_core/src/Polygon.cpp:32-44), which decides every cell a
// grid_map::PolygonIterator visits (LocalCostmap::bondingBoxHandle, M/src/local_costmap.cpp:860-922).
//
// Polygon table (built on the host by cilqr::build_polygon_table; only polygons that can touch the map are kept), n records:
//   table[0 .. 2n)   n cell ranges of four int32 {i_lo, i_hi, j_lo, j_hi}: the cells whose centres can lie inside the polygon's
//                    vertex bounding box, widened by a cell and clamped to the map.  A range is a cull only: it lets a
//                    wavefront skip a polygon, it never decides a cell.
//   table[2n ..)     n x V vertices (x, y).
// The cull reads the ranges 64 at a time, one per lane, and ballots: a polygon-by-polygon loop of wavefront-uniform reads is a
// chain of n dependent scalar-cache round trips per wavefront (n <= 1024), longer than the rest of the kernel.  The
// polygons that survive are visited in a wavefront-uniform loop over the ballot's bits, so their vertices are read with
// uniform addresses through the scalar cache and live in scalar registers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cilqr {

// Polygon::isInside for ROWS cells of one column (centres (px[k], py)), expression for expression: fp64, no contraction, IEEE
// division.  The cells share py, so an edge's crossing abscissa is formed once and compared with each px; bit k of the result
// is the parity of cell k's crossings.
template <int ROWS>
__device__ __forceinline__ unsigned polygon_is_inside(const double* __restrict__ vert, int V, const double (&px)[ROWS], double py) {
#pragma clang fp contract(off)
  unsigned odd = 0;
  double xj = vert[2 * (V - 1)], yj = vert[2 * (V - 1) + 1];
  for (int i = 0; i < V; ++i) {
    const double xi = vert[2 * i], yi = vert[2 * i + 1];
    if ((yi > py) != (yj > py)) {
      const double at = (xj - xi) * (py - yi) / (yj - yi) + xi;
#pragma unroll
      for (int k = 0; k < ROWS; ++k)
        if (px[k] < at) odd ^= 1u << k;
    }
    xj = xi;
    yj = yi;
  }
  return odd;
}

// ROWS cells of each of NJ columns (centres (px[k], py[c])) against every polygon of the table: bit k of hit[c] is set when at
// least one polygon contains the cell.  [i_first, i_last] x [j_first, j_last] must cover every cell the WAVEFRONT asks about.
// All 64 lanes of the wavefront must be active at the call (lane l reads the ranges of polygons l, l + 64, ... for all).
template <int ROWS, int NJ>
__device__ __forceinline__ void polygons_cover(const double* __restrict__ table, int n_polygons, int V, int i_first, int i_last, int j_first,
                                               int j_last, const double (&px)[ROWS], const double (&py)[NJ], unsigned (&hit)[NJ]) {
  const int4* __restrict__ ranges = reinterpret_cast<const int4*>(table);
  const double* __restrict__ vertices = table + 2 * (size_t)n_polygons;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NJ; ++c) hit[c] = 0;
  for (int base = 0; base < n_polygons; base += 64) {
    bool overlap = false;
    if (base + lane < n_polygons) {
      const int4 r = ranges[base + lane];
      overlap = !(r.x > i_last || r.y < i_first || r.z > j_last || r.w < j_first);
    }
    unsigned long long todo = __ballot(overlap);
    while (todo) {
      const int p = base + __builtin_ctzll(todo);
      todo &= todo - 1;
      const double* __restrict__ vert = vertices + (size_t)p * (2 * V);
#pragma unroll
      for (int c = 0; c < NJ; ++c) hit[c] |= polygon_is_inside<ROWS>(vert, V, px, py[c]);
    }
  }
}

}  // namespace cilqr
