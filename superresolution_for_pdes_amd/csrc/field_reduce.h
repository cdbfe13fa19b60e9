// The fp64 reductions of the field kernels (cascade.hip, tiled.hip, physics.hip, poisson_div.hip): one 256-thread
// block sum and block max, the grid sizes of a reduction and of an elementwise pass.  The bit-reproducibility these
// files promise rests on one fixed order -- the xor butterfly inside a wave, then the four waves as (0 + 1) + (2 + 3)
// -- so it is written once, here.  Everything is forceinline / inline: each translation unit gets its own copy.
// poisson.hip and poisson_rows.hip add their wave sums one after the other over a variable number of waves (some
// through agent-scope loads): they differ on purpose and keep their own reductions.
#pragma once
#include "common.h"

namespace srpde {

constexpr int kRedThreads = 256;
constexpr int kRedChunk = 2048;      // elements one workgroup takes per grid stride
constexpr int kRedMaxBlocks = 256;   // per (example, field): 640^2 -> 200 workgroups

// workgroups of a reduction over n elements
inline int red_blocks(long long n) {
  return (int)std::min<long long>(std::max<long long>((n + kRedChunk - 1) / kRedChunk, 1), kRedMaxBlocks);
}

// workgroups of 256 threads of a grid-stride pass over total elements
inline int elementwise_grid(long long total) {
  return (int)std::min<long long>(std::max<long long>((total + 255) / 256, 1), 8192);
}

// sum over the 256 threads of a block, the same bits on every thread; sh: 4 doubles, which the caller may read
// until its next barrier
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();   // the previous use of sh is over
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// maximum over the 256 threads of a block; sh as for block_sum.  In two halves for the kernels where one thread
// wants the value: every thread calls block_max_store, the thread that writes the partial reads block_max_load(sh)
// where it stores it (read earlier, the compiler schedules that thread's epilogue differently).
__device__ __forceinline__ void block_max_store(double v, double* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
}
__device__ __forceinline__ double block_max_load(const double* sh) {
  return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
__device__ __forceinline__ double block_max(double v, double* sh) {
  block_max_store(v, sh);
  return block_max_load(sh);
}

// the sum of nb partials in the one order every block uses: thread t adds part[t], part[t + 256], ..., then block_sum
__device__ __forceinline__ double resum(const double* part, int nb, double* sh) {
  double v = 0.0;
  for (int i = threadIdx.x; i < nb; i += kRedThreads) v += part[i];
  return block_sum(v, sh);
}

}  // namespace srpde
