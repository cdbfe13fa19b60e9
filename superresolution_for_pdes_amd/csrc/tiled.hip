// Overlapping-tile cascade level that needs no ground truth (tiled_inference.py), gfx950.
//
// cascade.hip cuts a field into disjoint tile^2 tiles and normalises with the next level's ground truth.  Here
// the windows overlap and the statistics come from what a user has -- the coarse solution and f / theta on the
// fine grid:
//   srpde_tiled_level_stats   u statistics from u_cur [E][S][S], f / theta statistics from the fine fields [2 launches]
//   srpde_tiled_assemble      window -> normalise -> bilinear x2 -> concat: the U-Net input                 [1 launch]
//   srpde_tiled_blend_denorm  U-Net output -> partition-of-unity blend -> denormalise -> fp64 field         [1 launch]
//
// Geometry, the same on both axes: window k of m = ceil((S - tile) / stride) + 1 starts at
// min(k stride, S - tile) on the coarse grid (the last one is clamped to the edge, so S need not be a multiple of
// anything) and covers [2 start, 2 start + 2 tile) on the fine grid.  Starts increase strictly.  Tile order:
// example-major, then row-major over the m x m windows, as in cascade.hip.
//
// Statistics and assemble are the same kernels as cascade.hip's (cascade_level.h): the statistics with two field
// lengths, each field reduced over red_blocks(its own length) workgroups, so a row is bit-equal to what
// srpde_cascade_level_stats gives for the same field; the assemble with the window origin above, which for
// stride == tile is the disjoint tile's (tests/test_gpu_tiled.py compares the bits of both).
//
// Blend: gather form, one thread per output pixel; the windows that cover it are visited in ascending tile
// order, num = sum w * (double)y and the integer den = sum w, w = w1(y) w1(x) with w1(i) = min(i + 1, 2 tile - i)
// ("linear") or 1 ("flat").  w < 2^28 and y has 24 significant bits, so every product is exact in fp64 (fused or
// not) and a pixel under one window gets that window's value back unchanged.  No atomics, no scatter.
#include "cascade_level.h"
#include "common.h"
#include "field_reduce.h"

#include <climits>

namespace srpde {

__device__ __forceinline__ int tiled_start(int k, int S, int tile, int stride) { return min(k * stride, S - tile); }

// the windows [lo, hi] that cover coarse position c: start_k <= c < start_k + tile.  Unclamped windows k <= m - 2
// need k stride <= c < k stride + tile; the last one (start S - tile) covers every c >= S - tile.
__device__ __forceinline__ void tiled_cover(int c, int S, int tile, int stride, int m, int& lo, int& hi) {
  lo = c < tile ? 0 : min((c - tile) / stride + 1, m - 1);
  hi = c >= S - tile ? m - 1 : c / stride;
}

// One thread per element of u_next [E][2S][2S], x fastest: a wave's reads of one window row are contiguous.
template <int kWindow>
__global__ __launch_bounds__(256) void tiled_blend_kernel(const float* __restrict__ yt, const float* __restrict__ stats,
                                                          int E, int S, int tile, int stride, int m,
                                                          double* __restrict__ u_next) {
  const int t2 = 2 * tile, S2 = 2 * S;
  const long long field = (long long)S2 * S2, total = (long long)E * field, plane = (long long)t2 * t2;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(q / field);
    const int pix = (int)(q - (long long)e * field), Y = pix / S2, X = pix - Y * S2;
    int ilo, ihi, jlo, jhi;
    tiled_cover(Y >> 1, S, tile, stride, m, ilo, ihi);
    tiled_cover(X >> 1, S, tile, stride, m, jlo, jhi);
    double num = 0.0;
    long long den = 0;
    for (int ti = ilo; ti <= ihi; ++ti) {
      const int y = Y - 2 * tiled_start(ti, S, tile, stride);
      const long long wy = kWindow == 0 ? min(y + 1, t2 - y) : 1;
      const float* row = yt + (((long long)e * m + ti) * m) * plane + (long long)y * t2;
      for (int tj = jlo; tj <= jhi; ++tj) {
        const int x = X - 2 * tiled_start(tj, S, tile, stride);
        const long long w = kWindow == 0 ? wy * min(x + 1, t2 - x) : 1;
        num += (double)w * (double)row[tj * plane + x];
        den += w;
      }
    }
    const float v = (float)(num / (double)den);
    u_next[q] = (double)denorm(v, stats[e * 6 + 1], stats[e * 6]);
  }
}

// m, or 0 for a bad geometry
static int tiled_m(int S, int tile, int stride) {
  if (stride < 1 || stride > tile || tile > S || S > 16384) return 0;
  return (S - tile + stride - 1) / stride + 1;
}

}  // namespace srpde

using namespace srpde;

// E > 0, the geometry valid and E m^2 within an int; sets m
#define TILED_CHECK_GEOMETRY(name)                                                             \
  const int m = tiled_m(S, tile, stride);                                                      \
  if (E <= 0 || m == 0 || (long long)E * m * m > INT_MAX)                                      \
    SRPDE_FAIL(kErrShape,                                                                      \
               name ": bad shape E=%d S=%d tile=%d stride=%d (1 <= stride <= tile <= S <= 16384, " \
                    "E m^2 in an int)",                                                        \
               E, S, tile, stride)

extern "C" {

int srpde_tiled_tiles_per_side(int S, int tile, int stride) {
  const int m = tiled_m(S, tile, stride);
  if (m == 0)
    SRPDE_FAIL(kErrShape,
               "srpde_tiled_tiles_per_side: bad geometry S=%d tile=%d stride=%d (1 <= stride <= tile <= S <= 16384)", S,
               tile, stride);
  return m;
}

size_t srpde_tiled_level_stats_workspace_size(int E, int S) {
  if (E <= 0 || S <= 0) return 0;
  return (size_t)E * 3 * red_blocks(4LL * S * S) * 2 * sizeof(double);
}

int srpde_tiled_level_stats(const double* u_cur, const double* f_next, const double* theta_next, int E, int S,
                            float* stats, int* theta_const, void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_cur && f_next && theta_next && stats && theta_const && workspace,
                  "srpde_tiled_level_stats: null pointer");
  if (E <= 0 || S <= 0 || S > 16384 || E > 65535)
    SRPDE_FAIL(kErrShape, "srpde_tiled_level_stats: bad shape E=%d S=%d", E, S);
  if (reinterpret_cast<uintptr_t>(workspace) & 7u)
    SRPDE_FAIL(kErrAlign, "srpde_tiled_level_stats: workspace not 8-byte aligned");
  if (ws_bytes < srpde_tiled_level_stats_workspace_size(E, S))
    SRPDE_FAIL(kErrWorkspace, "srpde_tiled_level_stats: workspace too small");
  const long long n_u = (long long)S * S;
  return level_stats_launch("srpde_tiled_level_stats", u_cur, f_next, theta_next, n_u, 4 * n_u, E, stats, theta_const,
                            static_cast<double*>(workspace), stream);
}

int srpde_tiled_assemble(const double* u_cur, const double* f_next, const double* theta_next, const float* stats,
                         int E, int S, int tile, int stride, float* x, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_cur && f_next && theta_next && stats && x, "srpde_tiled_assemble: null pointer");
  TILED_CHECK_GEOMETRY("srpde_tiled_assemble");
  return level_assemble_launch("srpde_tiled_assemble", u_cur, f_next, theta_next, stats, E, S, tile, stride, m, x,
                               stream);
}

int srpde_tiled_blend_denorm(const float* y, const float* stats, int E, int S, int tile, int stride, int window,
                             double* u_next, hipStream_t stream) {
  SRPDE_CHECK_ARG(y && stats && u_next, "srpde_tiled_blend_denorm: null pointer");
  TILED_CHECK_GEOMETRY("srpde_tiled_blend_denorm");
  if (window != 0 && window != 1)
    SRPDE_FAIL(kErrArg, "srpde_tiled_blend_denorm: window=%d (0 = linear, 1 = flat)", window);
  const long long total = (long long)E * (2 * S) * (2 * S);
  if (window == 0)
    hipLaunchKernelGGL(tiled_blend_kernel<0>, dim3(elementwise_grid(total)), dim3(256), 0, stream, y, stats, E, S, tile,
                       stride, m, u_next);
  else
    hipLaunchKernelGGL(tiled_blend_kernel<1>, dim3(elementwise_grid(total)), dim3(256), 0, stream, y, stats, E, S, tile,
                       stride, m, u_next);
  SRPDE_LAUNCH_CHECK("srpde_tiled_blend_denorm");
  return 0;
}

}  // extern "C"
