// What does a lone wavefront pay for one non-arithmetic instruction between two fp64 vector instructions?  (diagnostic tool, not
// part of the product).  The serial loops of the solve kernel (phases R and F) are one-lane chains on a wavefront that has its
// SIMD to itself; DESIGN.md §4.2 prices them at about 5 ticks per issued instruction of any kind, which tools/ubench_exec.hip
// measured for independent v_fma_f64 only.  Here: a stream of independent v_fma_f64 (four accumulators, round robin), and the
// same stream with ONE filler behind every v_fma_f64: s_add_i32, v_mov_b32 (from a scalar register, as the LDS store addresses
// of forward_smem are formed), v_add_u32 (a cursor bump), s_nop 0.  Ticks per added instruction = (variant - base) / fillers.
// Then the price of a pad by its length: s_nop N for N = 1 … 7 (N + 1 wait states) in the same place — does a shorter pad cost
// less than a longer one, or does only removing it count?
// One wavefront per SIMD (1024 blocks of 64 lanes on 256 CUs), s_memtime around 256 trips of 16 pairs.
//   hipcc -O3 --offload-arch=gfx950 -o tools/ubench_slot tools/ubench_slot.hip && tools/ubench_slot
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#define N_IT 256
#define R4(x) x x x x
#define FMA4(F)                                                                                                                  \
  asm volatile("v_fma_f64 %0, %7, %8, %9\n" F "v_fma_f64 %1, %8, %9, %7\n" F "v_fma_f64 %2, %9, %7, %8\n" F "v_fma_f64 %3, %7, %9, %8\n" F \
               : "=&v"(x4), "=&v"(x5), "=&v"(x6), "=&v"(x7), "+s"(sc), "+v"(vm), "+v"(va)                                          \
               : "v"(x0), "v"(x1), "v"(x2)                                                                                       \
               : "scc");
template <int KIND>
__global__ __launch_bounds__(64) void k(double* out, unsigned long long* cyc, double a, int s_in) {
  double x0 = a + threadIdx.x, x1 = a * 2, x2 = a * 3, x4 = a * 5, x5 = a * 6, x6 = a * 7, x7 = a * 8;
  int sc = s_in, vm = threadIdx.x, va = threadIdx.x;
  const unsigned long long t0 = __builtin_readcyclecounter();
  for (int i = 0; i < N_IT; ++i) {
    if (KIND == 0) { R4(FMA4("")) }
    if (KIND == 1) { R4(FMA4("s_add_i32 %4, %4, 16\n")) }
    if (KIND == 2) { R4(FMA4("v_mov_b32 %5, %4\n")) }
    if (KIND == 3) { R4(FMA4("v_add_u32 %6, 16, %6\n")) }
    if (KIND == 4) { R4(FMA4("s_nop 0\n")) }
    if (KIND == 5) { R4(FMA4("s_nop 1\n")) }
    if (KIND == 6) { R4(FMA4("s_nop 2\n")) }
    if (KIND == 7) { R4(FMA4("s_nop 3\n")) }
    if (KIND == 8) { R4(FMA4("s_nop 4\n")) }
    if (KIND == 9) { R4(FMA4("s_nop 5\n")) }
    if (KIND == 10) { R4(FMA4("s_nop 6\n")) }
    if (KIND == 11) { R4(FMA4("s_nop 7\n")) }
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  out[threadIdx.x + blockIdx.x * 64] = x0 + x1 + x2 + x4 + x5 + x6 + x7 + sc + vm + va;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}
template <int KIND> double run(const char* name, double base) {
  const int blocks = 1024;
  double* out; unsigned long long* cyc;
  if (hipMalloc(&out, 8 * 64 * blocks) != hipSuccess || hipMalloc(&cyc, 8 * blocks) != hipSuccess) { printf("hipMalloc failed\n"); exit(1); }
  for (int r = 0; r < 2; ++r) k<KIND><<<blocks, 64>>>(out, cyc, 1.0000001, 3);
  if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
  std::vector<unsigned long long> h(blocks);
  (void)hipMemcpy(h.data(), cyc, 8 * blocks, hipMemcpyDeviceToHost);
  double mean = 0, mn = 1e30;
  for (auto v : h) { mean += v; mn = v < mn ? (double)v : mn; }
  mean /= blocks;
  const double per = mean / N_IT / 16, per_min = mn / N_IT / 16;
  if (KIND == 0) printf("%-44s %6.2f ticks per v_fma_f64 (fastest wavefront %.2f)\n", name, per, per_min);
  else printf("%-44s %6.2f ticks per pair (fastest %.2f): %+.2f ticks per added instruction\n", name, per, per_min, per - base);
  (void)hipFree(out); (void)hipFree(cyc);
  return per;
}
int main() {
  const double base = run<0>("v_fma_f64 independent", 0.0);
  run<1>("  + s_add_i32 behind each", base);
  run<2>("  + v_mov_b32 (from SGPR) behind each", base);
  run<3>("  + v_add_u32 behind each", base);
  run<4>("  + s_nop 0 behind each", base);
  run<5>("  + s_nop 1 behind each", base);
  run<6>("  + s_nop 2 behind each", base);
  run<7>("  + s_nop 3 behind each", base);
  run<8>("  + s_nop 4 behind each", base);
  run<9>("  + s_nop 5 behind each", base);
  run<10>("  + s_nop 6 behind each", base);
  run<11>("  + s_nop 7 behind each", base);
  return 0;
}
