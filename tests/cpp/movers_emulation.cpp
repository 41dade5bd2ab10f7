// movers_emulation.cpp — the ownership rule of csrc/costmap_movers.hpp on the host: a sequential emulation of what one workgroup of
// costmap_movers.hip does per tile (the apron image, pass i, pass j), built by tests/test_clear_movers.py with
// -fsanitize=address,undefined and compared there with the brute-force definition.  Plain C++: no HIP, no device.
//
//   movers_emulation IN OUT
// IN: int32 records, one per case: rows, cols, halo2, n, then n ascending mover labels, then rows*cols labels, column-major.
// OUT: per case rows*cols owners and rows*cols squared distances to the nearest mover cell (-1: none within halo2).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "costmap_movers.hpp"

using namespace cilqr;

// what one workgroup does for the tile at (i0, j0), lane after lane; the buffers are exactly as large as the kernel's LDS blocks
static void tile(const std::vector<int32_t>& label, int rows, int cols, int halo2, const std::vector<int32_t>& movers, int i0, int j0,
                 std::vector<int32_t>& owner, std::vector<int32_t>& near) {
  const int r = cm_isqrt(halo2), WI = CM_TILE_I + 2 * r, HJ = CM_TILE_J + 2 * r;
  std::vector<int32_t> lab((size_t)WI * HJ);
  std::vector<uint32_t> words((size_t)CM_TILE_I * HJ);
  for (int at = 0; at < WI * HJ; ++at) {
    const int aj = at / WI, ai = at - aj * WI;
    const int i = i0 - r + ai, j = j0 - r + aj;
    int32_t v = -1;
    if (i >= 0 && i < rows && j >= 0 && j < cols) {
      const int32_t l = label[(size_t)j * rows + i];
      if (l >= 0) v = (l & CM_LABEL_MASK) | (cm_find_label(movers.data(), (int)movers.size(), l) ? CM_MOVER_BIT : 0);
    }
    lab[at] = v;
  }
  for (int at = 0; at < CM_TILE_I * HJ; ++at) words[at] = cm_pass_i(lab.data() + (size_t)(at / CM_TILE_I) * WI, at % CM_TILE_I, r);
  for (int lj = 0; lj < CM_TILE_J; ++lj)
    for (int li = 0; li < CM_TILE_I; ++li) {
      const int i = i0 + li, j = j0 + lj;
      if (i >= rows || j >= cols) continue;
      uint32_t key;
      int mover_d2;
      cm_pass_j(words.data(), li, lj, r, &key, &mover_d2);
      owner[(size_t)j * rows + i] = cm_owner(key, halo2);
      near[(size_t)j * rows + i] = mover_d2 <= halo2 ? mover_d2 : -1;
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
    const int rows = head[0], cols = head[1], halo2 = head[2], n = head[3];
    if (rows < 1 || cols < 1 || rows > 1024 || cols > 1024 || halo2 < 0 || halo2 > CILQR_CLEAR_MOVERS_MAX_HALO2 || n < 0 || n > 1024) return 3;
    const int cells = rows * cols;
    std::vector<int32_t> movers(n), label(cells), owner(cells, -5), near(cells, -5);
    if (n && fread(movers.data(), sizeof(int32_t), n, in) != (size_t)n) return 3;
    if (fread(label.data(), sizeof(int32_t), cells, in) != (size_t)cells) return 3;
    for (int j0 = 0; j0 < cols; j0 += CM_TILE_J)
      for (int i0 = 0; i0 < rows; i0 += CM_TILE_I) tile(label, rows, cols, halo2, movers, i0, j0, owner, near);
    if (fwrite(owner.data(), sizeof(int32_t), cells, out) != (size_t)cells || fwrite(near.data(), sizeof(int32_t), cells, out) != (size_t)cells) return 4;
    ++cases;
  }
  // the value key orders as the values do, and comes back
  const float vals[] = {-3.0e38f, -7.5f, -1e-40f, -0.0f, 0.0f, 1e-40f, 30.0f, 100.0f, 3.0e38f};
  for (size_t a = 0; a + 1 < sizeof vals / sizeof *vals; ++a) {
    const uint32_t ka = cm_value_key(vals[a]), kb = cm_value_key(vals[a + 1]);
    const bool equal = vals[a] == vals[a + 1];
    if (ka == 0 || kb == 0 || (equal ? ka != kb : !(ka < kb)) || cm_key_value(kb) != vals[a + 1]) return 5;
  }
  fclose(in);
  if (fclose(out) != 0) return 4;
  printf("%d cases\n", cases);
  return 0;
}
