// costmap_movers.hpp — the ownership rule of cilqr_clear_movers* (costmap_movers.hip; include/cilqr.h) as plain C++: the mover
// test of a row, the two separable passes over a tile's labels, the search among the mover labels and the key of a cell value.
// The kernel runs these functions over LDS; tests/cpp/movers_emulation.cpp runs the same functions on the host, tile after tile,
// under the address and undefined-behaviour sanitizers, and tests/test_clear_movers.py compares it with the brute-force definition.
//
// A tile is CM_TILE_I x CM_TILE_J cells; around it lies an apron of r = isqrt(halo2) cells.  `lab` holds the apron image,
// (CM_TILE_I + 2r) words a column: -1 for a cell that is not linked or lies outside the layer, else its label (< 2^20: rows and
// cols <= 1024) with CM_MOVER_BIT set where the label is a mover's.
//   pass i   for one column of the image and one i of the tile: the smallest (|di|, label) among the linked cells of the column
//            within |di| <= r, and the smallest |di| among the mover cells, packed into one word (cm_pass_i);
//   pass j   for one cell of the tile: over the 2r + 1 columns, the smallest (di² + dj², label) and the smallest mover di² + dj²
//            (cm_pass_j).
// For a fixed column dj is fixed, so di² + dj² grows with |di| and equal |di| means equal distance: the column's best (|di|, label)
// is the column's best (distance, label), and the minimum over the columns is the definition's minimum over the window.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "cilqr.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CILQR_CM_FN __host__ __device__ __forceinline__
#else
#define CILQR_CM_FN inline
#endif

namespace cilqr {

constexpr int CM_TILE_I = 64;  // along i: a wavefront's worth of consecutive words of the column-major layer
constexpr int CM_TILE_J = 16;
constexpr int CM_MAX_R = 32;   // isqrt(CILQR_CLEAR_MOVERS_MAX_HALO2)
constexpr int CM_LABEL_BITS = 20;
constexpr int32_t CM_LABEL_MASK = (1 << CM_LABEL_BITS) - 1;
constexpr int32_t CM_MOVER_BIT = 1 << 30;
constexpr uint32_t CM_NO_DI = 63;              // the |di| field of a column without a candidate
constexpr uint32_t CM_NO_KEY = 0xffffffffu;    // (distance << 20 | label) of a cell nobody reaches
constexpr int CM_NO_D2 = 1 << 20;              // above every di² + dj² of a window
static_assert(CM_MAX_R * CM_MAX_R == CILQR_CLEAR_MOVERS_MAX_HALO2 && (uint32_t)CM_MAX_R < CM_NO_DI, "a |di| up to r fits its six bits below CM_NO_DI");
static_assert(2 * CM_MAX_R * CM_MAX_R < (1 << (32 - CM_LABEL_BITS)), "a window's squared distance fits above the label's bits");

// the largest r with r·r <= halo2 (halo2 in [0, 1024])
CILQR_CM_FN int cm_isqrt(int halo2) {
  int r = 0;
  while ((r + 1) * (r + 1) <= halo2) ++r;
  return r;
}

// Tracker form: is row k, whose comp label is `label`, a mover?  `slot` = assign[k]; `state` the M state rows of the layer.
CILQR_CM_FN bool cm_tracker_mover(double label, int k, int slot, int M, const double* state, int min_hits, double v_clear) {
  if (!(label >= 0.0) || slot < 0 || slot >= M) return false;
  const double* s = state + (size_t)slot * CILQR_TRACK_STATE;
  if (!(s[CILQR_TS_ID] >= 0.0) || s[CILQR_TS_DET] != (double)k || !(s[CILQR_TS_HITS] >= (double)min_hits)) return false;
  return hypot(s[CILQR_TS_VX], s[CILQR_TS_VY]) >= v_clear;  // (a NaN fails)
}

// n ascending labels: is `label` among them?
CILQR_CM_FN bool cm_find_label(const int32_t* sorted, int n, int32_t label) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted[mid] < label) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && sorted[lo] == label;
}

// One column of the apron image (`column` points at its first word, the image row i0 - r) and the tile row li: the word
// |di| of the nearest mover cell << 26 | |di| of the best linked cell << 20 | that cell's label.
CILQR_CM_FN uint32_t cm_pass_i(const int32_t* column, int li, int r) {
  uint32_t best = (CM_NO_DI << CM_LABEL_BITS) | (uint32_t)CM_LABEL_MASK, mover = CM_NO_DI;
  for (int di = -r; di <= r; ++di) {
    const int32_t v = column[li + r + di];
    if (v < 0) continue;
    const uint32_t adi = (uint32_t)(di < 0 ? -di : di);
    const uint32_t key = (adi << CM_LABEL_BITS) | (uint32_t)(v & CM_LABEL_MASK);
    best = key < best ? key : best;
    if (v & CM_MOVER_BIT) mover = adi < mover ? adi : mover;
  }
  return (mover << 26) | best;
}

// The cell (li, lj) of the tile over the 2r + 1 columns of pass i (`words` holds CM_TILE_I words a column of the image, first the
// image column j0 - r): *key = distance << 20 | label of the best linked cell of the window (CM_NO_KEY: none), *mover_d2 the
// squared distance of the nearest mover cell (CM_NO_D2: none).
CILQR_CM_FN void cm_pass_j(const uint32_t* words, int li, int lj, int r, uint32_t* key, int* mover_d2) {
  uint32_t best = CM_NO_KEY;
  int mover = CM_NO_D2;
  for (int dj = -r; dj <= r; ++dj) {
    const uint32_t w = words[li + (lj + r + dj) * CM_TILE_I];
    const int adi = (int)(w >> CM_LABEL_BITS & 63u), amv = (int)(w >> 26);
    if (adi != (int)CM_NO_DI) {
      const uint32_t k = ((uint32_t)(adi * adi + dj * dj) << CM_LABEL_BITS) | (w & (uint32_t)CM_LABEL_MASK);
      best = k < best ? k : best;
    }
    if (amv != (int)CM_NO_DI) {
      const int d2 = amv * amv + dj * dj;
      mover = d2 < mover ? d2 : mover;
    }
  }
  *key = best;
  *mover_d2 = mover;
}

// the owner a key names under halo2: its label, or -1
CILQR_CM_FN int32_t cm_owner(uint32_t key, int halo2) {
  return key != CM_NO_KEY && (int)(key >> CM_LABEL_BITS) <= halo2 ? (int32_t)(key & (uint32_t)CM_LABEL_MASK) : -1;
}

// A finite value as an unsigned word that orders as the values do (-0 counts as +0), never 0; and back.
CILQR_CM_FN uint32_t cm_value_key(float v) {
  if (v == 0.0f) v = 0.0f;
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
CILQR_CM_FN float cm_key_value(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  memcpy(&v, &u, sizeof v);
  return v;
}

}  // namespace cilqr
