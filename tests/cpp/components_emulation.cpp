// components_emulation.cpp — the union and find steps of csrc/costmap_components.hpp on the host: a sequential emulation of the tile
// and seam launches of costmap_components.hip, built by tests/test_map_obstacles.py with -fsanitize=address,undefined and compared
// there with the flood fill.  Plain C++: no HIP, no device.
//
//   components_emulation IN OUT
// IN: int32 records, one per case: rows, cols, gap2, four, then rows*cols values of d2, column-major.  OUT: per case rows*cols labels
// and one int32, the overrun flag.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "costmap_components.hpp"

using namespace cilqr;

static bool linked(int d2, int gap2) { return d2 != INT_MAX && d2 <= gap2; }

// what one workgroup of the tiles launch does, lane after lane
static void tile(const std::vector<int32_t>& d2, int rows, int cols, int gap2, int nk, int i0, int j0, std::vector<int32_t>& label, int* overrun) {
  int lab[CC_TILE_I * CC_TILE_J];
  for (int lj = 0; lj < CC_TILE_J; ++lj)
    for (int li = 0; li < CC_TILE_I; ++li) {
      const int i = i0 + li, j = j0 + lj;
      const bool on = i < rows && j < cols && linked(d2[(size_t)j * rows + i], gap2);
      lab[li + lj * CC_TILE_I] = on ? li + lj * CC_TILE_I : -1;
    }
  for (int lj = 0; lj < CC_TILE_J; ++lj)
    for (int li = 0; li < CC_TILE_I; ++li) {
      const int loc = li + lj * CC_TILE_I;
      if (lab[loc] < 0) continue;
      for (int n = 0; n < nk; ++n) {
        int di, dj;
        cc_neighbour(n, &di, &dj);
        const int ni = li + di, nj = lj + dj;
        if (ni < 0 || ni >= CC_TILE_I || nj < 0) continue;
        const int other = ni + nj * CC_TILE_I;
        if (lab[other] >= 0) cc_union<CcHostMem>(lab, loc, other, CC_TILE_I * CC_TILE_J, overrun);
      }
    }
  for (int lj = 0; lj < CC_TILE_J; ++lj)
    for (int li = 0; li < CC_TILE_I; ++li) {
      const int i = i0 + li, j = j0 + lj;
      if (i >= rows || j >= cols) continue;
      int out = -1;
      if (lab[li + lj * CC_TILE_I] >= 0) {
        const int r = cc_find<CcHostMem>(lab, li + lj * CC_TILE_I, CC_TILE_I * CC_TILE_J, overrun);
        out = (i0 + r % CC_TILE_I) + (j0 + r / CC_TILE_I) * rows;
      }
      label[(size_t)j * rows + i] = out;
    }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[4];
  int cases = 0;
  while (fread(head, sizeof(int32_t), 4, in) == 4) {
    const int rows = head[0], cols = head[1], gap2 = head[2], nk = head[3] ? 2 : CC_NEIGHBOURS;
    if (rows < 1 || cols < 1 || rows > 1024 || cols > 1024) return 3;
    const int cells = rows * cols;
    std::vector<int32_t> d2(cells), label(cells);
    if (fread(d2.data(), sizeof(int32_t), cells, in) != (size_t)cells) return 3;
    int overrun = 0;
    for (int j0 = 0; j0 < cols; j0 += CC_TILE_J)
      for (int i0 = 0; i0 < rows; i0 += CC_TILE_I) tile(d2, rows, cols, gap2, nk, i0, j0, label, &overrun);
    // the seams launch, lane = cell
    int* P = label.data();
    for (int c = 0; c < cells; ++c) {
      const int i = c % rows, j = c / rows;
      if (P[c] < 0) continue;
      for (int n = 0; n < nk; ++n) {
        int di, dj;
        cc_neighbour(n, &di, &dj);
        const int ni = i + di, nj = j + dj;
        if (ni < 0 || ni >= rows || nj < 0) continue;
        if (ni / CC_TILE_I == i / CC_TILE_I && nj / CC_TILE_J == j / CC_TILE_J) continue;
        const int other = ni + nj * rows;
        if (P[other] >= 0) cc_union<CcHostMem>(P, c, other, cells, &overrun);
      }
    }
    // flatten
    for (int c = 0; c < cells; ++c)
      if (P[c] >= 0) P[c] = cc_find<CcHostMem>(P, c, cells, &overrun);
    const int32_t flag = overrun;
    if (fwrite(P, sizeof(int32_t), cells, out) != (size_t)cells || fwrite(&flag, sizeof(int32_t), 1, out) != 1) return 4;
    ++cases;
  }
  fclose(in);
  if (fclose(out) != 0) return 4;
  printf("%d cases\n", cases);
  return 0;
}
