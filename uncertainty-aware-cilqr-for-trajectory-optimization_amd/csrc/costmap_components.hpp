// costmap_components.hpp — the union and find steps of the component labelling (costmap_components.hip; cilqr_map_obstacles*,
// include/cilqr.h).  Plain C++ over a memory policy, so that the same two functions run in LDS, in device memory and — with
// CcHostMem — on the host, where tests/cpp/components_emulation.cpp drives them through a sequential emulation of the tile and
// seam launches under the address and undefined-behaviour sanitizers.
//
// A label array P holds, for a linked cell c, a parent P[c] <= c of the same component (P[c] == c: a root) and -1 elsewhere.
// Parents only ever decrease, so there is no cycle, a root is the lowest index of its set, and once every pair of neighbouring
// linked cells has been united the root of a cell is the lowest linear index of its component: the canonical label.
//
// Every loop carries the bound `limit` (rows·cols: no chain is longer).  On overrun *overrun is set and the function returns
// what it holds: the caller reports an error, a bug never spins.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CILQR_CC_FN __host__ __device__ __forceinline__
#else
#define CILQR_CC_FN inline
#endif

namespace cilqr {

// the host's memory: one thread, plain loads and stores
struct CcHostMem {
  static int load(const int* p) { return *p; }
  static int fetch_min(int* p, int v) {
    const int old = *p;
    if (v < old) *p = v;
    return old;
  }
};

template <typename Mem>
CILQR_CC_FN int cc_find(int* P, int c, int limit, int* overrun) {
  for (int n = 0; n <= limit; ++n) {
    const int up = Mem::load(P + c);
    if (up == c) return c;
    c = up;
  }
  *overrun = 1;
  return c;
}

// Unites the sets of the linked cells a and b.  The larger root is hung below the smaller by an atomic minimum; where another
// union got there first (the old value is not the root we saw), the pair (old parent, smaller root) remains to be united.
template <typename Mem>
CILQR_CC_FN void cc_union(int* P, int a, int b, int limit, int* overrun) {
  for (int n = 0; n <= limit; ++n) {
    a = cc_find<Mem>(P, a, limit, overrun);
    b = cc_find<Mem>(P, b, limit, overrun);
    if (a == b || *overrun) return;
    if (a < b) { const int t = a; a = b; b = t; }  // a > b
    const int old = Mem::fetch_min(P + a, b);
    if (old == a) return;
    a = old;
  }
  *overrun = 1;
}

// The lower neighbours of cell (i, j) in column-major order — the ones whose index is below i + j*rows — as (di, dj):
// 4-connectivity takes the first two, 8-connectivity all four.
constexpr int CC_NEIGHBOURS = 4;
CILQR_CC_FN void cc_neighbour(int k, int* di, int* dj) {
  *di = k == 0 ? -1 : k == 1 ? 0 : k == 2 ? -1 : 1;
  *dj = k == 0 ? 0 : -1;
}

// tile of the first launch: TILE_I cells along i (a wavefront's worth: lanes along i load consecutive words) by TILE_J along j
constexpr int CC_TILE_I = 64;
constexpr int CC_TILE_J = 16;

}  // namespace cilqr
