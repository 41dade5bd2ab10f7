// costmap_movers.hip — the static layer (cilqr_clear_movers*, include/cilqr.h): the cells of L layers that belong to components
// which moving tracks own are set to `fill`, so that a vehicle the tracks already predict does not also stand in the map for the
// whole horizon.  The ownership rule is that of costmap_movers.hpp; this file stages what it reads and counts what it decides.
//
// One clear of `fields` and two launches:
//   tiles    one workgroup of CLEAR_MOVERS_THREADS lanes per CM_TILE_I x CM_TILE_J tile, layer slowest; lane along i, four cells a lane.
//            prologue  lane = row: which of the K rows are movers (tracker or mask form); their labels go to LDS in ascending order
//                      (each mover row counts the mover labels below its own: K is small and movers are few).
//            stage     the labels of the tile and an apron of r = isqrt(halo2) cells go to LDS, a mover's label with CM_MOVER_BIT.
//            pass i    lane = (i of the tile, column of the image): one word per pair (cm_pass_i).
//            pass j    lane = cell: the owner and the nearest mover cell (cm_pass_j); the cell is written, owner_out too.
//            counts    a butterfly per wavefront, the first lane over the wavefronts' records, then ONE 64-bit integer atomic
//                      per field and workgroup into the layer's row of `fields`: sums, and a maximum of (value key, ~cell).
//   finish   lane = layer: the raw integers become the doubles of the row.
// Integer sums and one integer maximum: no order changes a bit, a layer's bits depend on that layer alone.  No float atomics, no
// scratch memory, nothing allocated.
// LDS (dynamic, words): [sorted: K'][image: (CM_TILE_I + 2r)(CM_TILE_J + 2r)][pass i: CM_TILE_I·(CM_TILE_J + 2r)], K' = K rounded
// up to even; the rows' raw labels and, at the end, the wavefronts' records lie over the pass-i words.  64 KiB at K = 1024, r = 32
// (the counting barrier of the prologue keeps 256 bytes of its own beside them).
#include "cilqr_rollout_core.hpp"
#include "costmap_movers.hpp"

namespace cilqr {

using dev::kernel_args;

namespace {

constexpr int F = CILQR_CLEAR_MOVERS_FIELDS;
constexpr int WAVES = CLEAR_MOVERS_THREADS / 64;
constexpr int PER_LANE = CM_TILE_I * CM_TILE_J / CLEAR_MOVERS_THREADS, STEP_J = CLEAR_MOVERS_THREADS / CM_TILE_I;
constexpr int N_COUNTS = 5;  // cleared, owned linked, owned halo, contested, kept unknown

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// grid L·ceil(rows/CM_TILE_I)·ceil(cols/CM_TILE_J), layer slowest
__global__ __launch_bounds__(CLEAR_MOVERS_THREADS) void cilqr_clear_movers_kernel(ClearMoversArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t clear_movers_lds[];
  const int tid = threadIdx.x;
  const int rows = a.rows, cols = a.cols, K = a.K, r = a.r;
  const int WI = CM_TILE_I + 2 * r, HJ = CM_TILE_J + 2 * r;
  int32_t* sorted = clear_movers_lds;                      // [K']
  int32_t* lab = sorted + ((K + 1) & ~1);                  // [HJ][WI]
  uint32_t* words = (uint32_t*)(lab + WI * HJ);            // [HJ][CM_TILE_I]
  int32_t* raw = (int32_t*)words;                          // [K], until pass i
  unsigned long long* rec = (unsigned long long*)words;    // [WAVES][N_COUNTS + 1], after pass j
  const int ti_n = (rows + CM_TILE_I - 1) / CM_TILE_I, tj_n = (cols + CM_TILE_J - 1) / CM_TILE_J;
  const int l = blockIdx.x / (ti_n * tj_n), t = blockIdx.x - l * (ti_n * tj_n);
  const int i0 = (t % ti_n) * CM_TILE_I, j0 = (t / ti_n) * CM_TILE_J;
  const size_t cells = (size_t)rows * cols, base = (size_t)l * cells;

  // ---- prologue: the movers among the K rows
  // (each phase reads what it needs of the arguments through a pointer the compiler cannot trace back to the preloaded ones:
  // nothing but the tile's few integers is carried in scalar registers from phase to phase)
  int n_mov = 0;
  {
    const ClearMoversArgs& q = kernel_args<ClearMoversArgs>();
    const double* comp = q.comp + (size_t)l * K * CILQR_MAP_OBSTACLE_FIELDS;
    // (the trip count is the workgroup's, so that every lane meets the counting barrier)
    for (int k0 = 0; k0 < K; k0 += CLEAR_MOVERS_THREADS) {
      const int k = k0 + tid;
      bool mover = false;
      if (k < K) {
        const double c = comp[(size_t)k * CILQR_MAP_OBSTACLE_FIELDS + CILQR_MO_LABEL];
        if (q.mask) mover = c >= 0.0 && q.mask[(size_t)l * K + k] != 0;
        else mover = cm_tracker_mover(c, k, q.assign[(size_t)l * K + k], q.M, q.state + (size_t)l * q.M * CILQR_TRACK_STATE, q.min_hits, q.v_clear);
        // (a label beyond every cell's matches none: it only counts as a row)
        raw[k] = mover ? (c < (double)(CM_LABEL_MASK + 1) ? (int32_t)c : CM_LABEL_MASK + 1) : -1;
      }
      n_mov += __syncthreads_count(mover ? 1 : 0);
    }
    __syncthreads();
    for (int k = tid; k < K; k += CLEAR_MOVERS_THREADS) {
      const int32_t mine = raw[k];
      if (mine < 0) continue;
      int rank = 0;
      for (int o = 0; o < K; ++o) {
        const int32_t v = raw[o];
        rank += v >= 0 && (v < mine || (v == mine && o < k)) ? 1 : 0;
      }
      sorted[rank] = mine;
    }
    __syncthreads();
  }

  // ---- stage: the image of the tile and its apron
  for (int at = tid; at < WI * HJ; at += CLEAR_MOVERS_THREADS) {
    const int aj = at / WI, ai = at - aj * WI;
    const int i = i0 - r + ai, j = j0 - r + aj;
    int32_t v = -1;
    if (i >= 0 && i < rows && j >= 0 && j < cols) {
      const int32_t label = kernel_args<ClearMoversArgs>().label[base + (size_t)j * rows + i];
      if (label >= 0) v = (label & CM_LABEL_MASK) | (cm_find_label(sorted, n_mov, label) ? CM_MOVER_BIT : 0);
    }
    lab[at] = v;
  }
  __syncthreads();  // (the sort has read `raw` before the barrier above: pass i may write over it)

  // ---- pass i
  for (int at = tid; at < CM_TILE_I * HJ; at += CLEAR_MOVERS_THREADS) words[at] = cm_pass_i(lab + (at / CM_TILE_I) * WI, at % CM_TILE_I, r);
  __syncthreads();

  // ---- pass j, and the cells
  int n[N_COUNTS] = {0, 0, 0, 0, 0};
  unsigned long long top = 0ull;
  {
    const ClearMoversArgs& q = kernel_args<ClearMoversArgs>();
    const int li = tid % CM_TILE_I, lj0 = tid / CM_TILE_I, i = i0 + li;
    const uint32_t fill_bits = __float_as_uint(q.fill);
    for (int k = 0; k < PER_LANE; ++k) {
      const int lj = lj0 + k * STEP_J, j = j0 + lj;
      if (i >= rows || j >= cols) continue;
      uint32_t key;
      int mover_d2;
      cm_pass_j(words, li, lj, r, &key, &mover_d2);
      const int32_t owner = cm_owner(key, q.halo2);
      const bool linked = lab[(li + r) + (lj + r) * WI] >= 0;
      const bool owned = owner >= 0 && cm_find_label(sorted, n_mov, owner);
      const size_t c = (size_t)j * rows + i;
      const uint32_t in_bits = __float_as_uint(q.layer[(size_t)l * (size_t)q.layer_stride + c]);
      const float v = __uint_as_float(in_bits);
      uint32_t out_bits = in_bits;
      if (owned) {
        n[1] += linked ? 1 : 0;
        n[2] += linked ? 0 : 1;
        if (v != v) n[4] += 1;
        else {
          out_bits = fill_bits;
          if (v - v == 0.0f) {  // finite
            const unsigned long long mine = (unsigned long long)cm_value_key(v) << 32 | (unsigned long long)(0xffffffffu - (uint32_t)c);
            top = mine > top ? mine : top;
          }
        }
      } else if (!linked && mover_d2 <= q.halo2) {
        n[3] += 1;
      }
      n[0] += out_bits != in_bits ? 1 : 0;
      q.layer_out[base + c] = __uint_as_float(out_bits);
      if (q.owner_out) q.owner_out[base + c] = owner;
    }
  }

  // ---- the workgroup's record
  for (int f = 0; f < N_COUNTS; ++f) n[f] = wave_sum(n[f]);
  top = wave_max(top);
  __syncthreads();  // every lane is through with the pass-i words
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
    for (int f = 0; f < N_COUNTS; ++f) rec[wave * (N_COUNTS + 1) + f] = (unsigned long long)n[f];
    rec[wave * (N_COUNTS + 1) + N_COUNTS] = top;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < WAVES; ++w) {
    for (int f = 0; f < N_COUNTS; ++f) n[f] += (int)rec[w * (N_COUNTS + 1) + f];
    const unsigned long long o = rec[w * (N_COUNTS + 1) + N_COUNTS];
    top = o > top ? o : top;
  }
  unsigned long long* out = (unsigned long long*)(kernel_args<ClearMoversArgs>().fields + (size_t)l * F);
  if (t == 0 && n_mov) atomicAdd(out + CILQR_CM_MOVERS, (unsigned long long)n_mov);
  if (n[0]) atomicAdd(out + CILQR_CM_CLEARED, (unsigned long long)n[0]);
  if (n[1]) atomicAdd(out + CILQR_CM_OWNED_LINKED, (unsigned long long)n[1]);
  if (n[2]) atomicAdd(out + CILQR_CM_OWNED_HALO, (unsigned long long)n[2]);
  if (n[3]) atomicAdd(out + CILQR_CM_CONTESTED, (unsigned long long)n[3]);
  if (n[4]) atomicAdd(out + CILQR_CM_KEPT_UNKNOWN, (unsigned long long)n[4]);
  if (top) atomicMax(out + CILQR_CM_MAX_VALUE, top);
}

// grid ceil(L / CLEAR_MOVERS_THREADS), lane = layer
__global__ __launch_bounds__(CLEAR_MOVERS_THREADS) void cilqr_clear_movers_finish_kernel(ClearMoversArgs a) {
  const int l = blockIdx.x * CLEAR_MOVERS_THREADS + threadIdx.x;
  if (l >= a.L) return;
  double* row = a.fields + (size_t)l * F;
  unsigned long long v[F];
  for (int f = 0; f < F; ++f) v[f] = ((const unsigned long long*)row)[f];
  const unsigned long long top = v[CILQR_CM_MAX_VALUE];
  for (int f = 0; f < F; ++f) row[f] = (double)v[f];
  row[CILQR_CM_MAX_VALUE] = top ? (double)cm_key_value((uint32_t)(top >> 32)) : -1.0;
  row[CILQR_CM_MAX_CELL] = top ? (double)(0xffffffffu - (uint32_t)top) : -1.0;
}

}  // namespace

size_t clear_movers_lds_bytes(int K, int r) {
  const size_t WI = CM_TILE_I + 2 * (size_t)r, HJ = CM_TILE_J + 2 * (size_t)r;
  return (((size_t)K + 1) / 2 * 2 + WI * HJ + CM_TILE_I * HJ) * sizeof(int32_t);
}

hipError_t launch_clear_movers(const ClearMoversArgs& a, hipStream_t stream) {
  if (a.L <= 0) return hipSuccess;
  // (the host checked that the grid stays below 2^31 workgroups)
  const unsigned tiles = (unsigned)((a.rows + CM_TILE_I - 1) / CM_TILE_I) * (unsigned)((a.cols + CM_TILE_J - 1) / CM_TILE_J);
  hipError_t e = hipMemsetAsync(a.fields, 0, (size_t)a.L * F * sizeof(double), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_clear_movers_kernel, dim3(tiles * (unsigned)a.L), dim3(CLEAR_MOVERS_THREADS), clear_movers_lds_bytes(a.K, a.r), stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cilqr_clear_movers_finish_kernel, dim3(((unsigned)a.L + CLEAR_MOVERS_THREADS - 1) / CLEAR_MOVERS_THREADS),
                     dim3(CLEAR_MOVERS_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cilqr
