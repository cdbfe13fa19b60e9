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
// Statistics: every field is reduced exactly as cascade_stats_partial_kernel / _final_kernel reduce a field of
// its own length n -- red_blocks(n) workgroups striding over it, deviations from its first value, the xor
// butterfly, the four waves in order, the partials summed in index order -- so a row is bit-equal to what
// srpde_cascade_level_stats gives for the same field.  kRed* and the two kernels' arithmetic mirror cascade.hip
// (tests/test_gpu_tiled.py compares the bits).
//
// Blend: gather form, one thread per output pixel; the windows that cover it are visited in ascending tile
// order, num = sum w * (double)y and the integer den = sum w, w = w1(y) w1(x) with w1(i) = min(i + 1, 2 tile - i)
// ("linear") or 1 ("flat").  w < 2^28 and y has 24 significant bits, so every product is exact in fp64 (fused or
// not) and a pixel under one window gets that window's value back unchanged.  No atomics, no scatter.
#include "common.h"
#include "resample.h"

#include <climits>

namespace srpde {

constexpr int kTiledRedThreads = 256;
constexpr int kTiledRedChunk = 2048;
constexpr int kTiledRedMaxBlocks = 256;

static int tiled_red_blocks(long long n) {
  return (int)std::min<long long>(std::max<long long>((n + kTiledRedChunk - 1) / kTiledRedChunk, 1),
                                  kTiledRedMaxBlocks);
}

__device__ __forceinline__ double tiled_block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();   // the previous use of sh is over
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// grid (nb_fine, 3 fields, E); field 0 = u_cur (n_u values, nb_u workgroups; the others leave at once), fields
// 1 / 2 = f / theta (n_f values, nb_fine workgroups): part[((e * 3 + fld) * nb_fine + b) * 2] = {sum d, sum d^2}
__global__ __launch_bounds__(kTiledRedThreads) void tiled_stats_partial_kernel(const double* __restrict__ u,
                                                                               const double* __restrict__ f,
                                                                               const double* __restrict__ th,
                                                                               long long n_u, int nb_u, long long n_f,
                                                                               double* __restrict__ part) {
  __shared__ double sh[4];
  const int fld = blockIdx.y, e = blockIdx.z;
  const long long n = fld == 0 ? n_u : n_f;
  const int nb = fld == 0 ? nb_u : (int)gridDim.x;
  if ((int)blockIdx.x >= nb) return;   // the whole workgroup
  const double* x = (fld == 0 ? u : fld == 1 ? f : th) + (long long)e * n;
  const double K = (double)(float)x[0];
  double s1 = 0.0, s2 = 0.0;
  for (long long i = (long long)blockIdx.x * kTiledRedThreads + threadIdx.x; i < n;
       i += (long long)nb * kTiledRedThreads) {
    const double d = (double)(float)x[i] - K;
    s1 += d;
    s2 += d * d;
  }
  s1 = tiled_block_sum(s1, sh);
  s2 = tiled_block_sum(s2, sh);
  if (threadIdx.x == 0) {
    double* p = part + (((long long)e * 3 + fld) * gridDim.x + blockIdx.x) * 2;
    p[0] = s1;
    p[1] = s2;
  }
}

// grid E, one wave: the partials of each field in index order -> the example's statistics row and theta flag
__global__ __launch_bounds__(64) void tiled_stats_final_kernel(const double* __restrict__ u,
                                                               const double* __restrict__ f,
                                                               const double* __restrict__ th, long long n_u, int nb_u,
                                                               long long n_f, int nb_f,
                                                               const double* __restrict__ part,
                                                               float* __restrict__ stats,
                                                               int* __restrict__ theta_const) {
  const int e = blockIdx.x, lane = threadIdx.x;
#pragma unroll
  for (int fld = 0; fld < 3; ++fld) {
    const long long n = fld == 0 ? n_u : n_f;
    const int nb = fld == 0 ? nb_u : nb_f;
    const double* x = (fld == 0 ? u : fld == 1 ? f : th) + (long long)e * n;
    const double K = (double)(float)x[0];
    const double* p = part + ((long long)e * 3 + fld) * nb_f * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int j = lane; j < nb; j += 64) {
      s1 += p[2 * j];
      s2 += p[2 * j + 1];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
      const double dn = (double)n;
      const double mean = K + s1 / dn;
      const double var = fmax(s2 - s1 * s1 / dn, 0.0) / (dn - 1.0);   // unbiased, as torch.std
      float m = (float)mean, s = (float)sqrt(var);
      if (fld == 2) {   // GlobalNormalization: theta counts as constant when its fp32 std < 1e-6, then passes through
        const int c = s < 1e-6f ? 1 : 0;
        theta_const[e] = c;
        if (c) { m = 0.f; s = 1.f; }
      }
      stats[e * 6 + 2 * fld] = m;
      stats[e * 6 + 2 * fld + 1] = s;
    }
  }
}

__device__ __forceinline__ int tiled_start(int k, int S, int tile, int stride) { return min(k * stride, S - tile); }

// cascade_assemble_kernel with the window origin at tiled_start: one thread per element of x [T][3][2 tile][2 tile],
// the same expressions element for element (fp32 subtract, correctly rounded divide, the spelt-out contraction)
__global__ __launch_bounds__(256) void tiled_assemble_kernel(const double* __restrict__ u_cur,
                                                             const double* __restrict__ f_next,
                                                             const double* __restrict__ th_next,
                                                             const float* __restrict__ stats, int E, int S, int tile,
                                                             int stride, int m, float* __restrict__ xo) {
  const int t2 = 2 * tile, S2 = 2 * S;
  const long long plane = (long long)t2 * t2, total = (long long)E * m * m * plane;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const long long t = q / plane;
    const int pix = (int)(q - t * plane), y = pix / t2, x = pix - y * t2;
    const int e = (int)(t / (m * m)), r = (int)(t - (long long)e * m * m), ti = r / m, tj = r - ti * m;
    const int sy = tiled_start(ti, S, tile, stride), sx = tiled_start(tj, S, tile, stride);
    const float* st = stats + e * 6;
    const float um = st[0], us = st[1], fm = st[2], fs = st[3], tm = st[4], ts = st[5];
    const Lerp ly = lerp_index(y, tile, t2), lx = lerp_index(x, tile, t2);
    const double* base = u_cur + ((long long)e * S + sy) * S + sx;
    const float a = ((float)base[(long long)ly.i0 * S + lx.i0] - um) / us;
    const float b = ((float)base[(long long)ly.i0 * S + lx.i1] - um) / us;
    const float d = ((float)base[(long long)ly.i1 * S + lx.i0] - um) / us;
    const float f = ((float)base[(long long)ly.i1 * S + lx.i1] - um) / us;
    const long long fine = ((long long)e * S2 + 2 * sy + y) * S2 + 2 * sx + x;
    float* o = xo + t * 3 * plane + pix;
    // the contraction of cascade_assemble_kernel (one product rounded, the other fused, three times)
    float up;
    {
#pragma clang fp contract(off)
      const float top = __builtin_fmaf(lx.l1, b, lx.l0 * a);
      const float bot = __builtin_fmaf(lx.l1, f, lx.l0 * d);
      up = __builtin_fmaf(ly.l0, top, ly.l1 * bot);
    }
    o[0] = up;
    o[plane] = ((float)th_next[fine] - tm) / ts;
    o[2 * plane] = ((float)f_next[fine] - fm) / fs;
  }
}

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
    const float us = stats[e * 6 + 1], um = stats[e * 6];
    float r;
    {
#pragma clang fp contract(off)
      r = v * us;
      r = r + um;
    }
    u_next[q] = (double)r;
  }
}

static int tiled_grid(long long total) {
  return (int)std::min<long long>(std::max<long long>((total + 255) / 256, 1), 8192);
}

// m, or 0 for a bad geometry
static int tiled_m(int S, int tile, int stride) {
  if (stride < 1 || stride > tile || tile > S || S > 16384) return 0;
  return (S - tile + stride - 1) / stride + 1;
}

}  // namespace srpde

using namespace srpde;

#define TILED_FAIL(code, ...)        \
  do {                               \
    ::srpde::set_error(__VA_ARGS__); \
    return code;                     \
  } while (0)

// E > 0, the geometry valid and E m^2 within an int; sets m
#define TILED_CHECK_GEOMETRY(name)                                                             \
  const int m = tiled_m(S, tile, stride);                                                      \
  if (E <= 0 || m == 0 || (long long)E * m * m > INT_MAX)                                      \
    TILED_FAIL(kErrShape,                                                                      \
               name ": bad shape E=%d S=%d tile=%d stride=%d (1 <= stride <= tile <= S <= 16384, " \
                    "E m^2 in an int)",                                                        \
               E, S, tile, stride)

extern "C" {

int srpde_tiled_tiles_per_side(int S, int tile, int stride) {
  const int m = tiled_m(S, tile, stride);
  if (m == 0)
    TILED_FAIL(kErrShape,
               "srpde_tiled_tiles_per_side: bad geometry S=%d tile=%d stride=%d (1 <= stride <= tile <= S <= 16384)", S,
               tile, stride);
  return m;
}

size_t srpde_tiled_level_stats_workspace_size(int E, int S) {
  if (E <= 0 || S <= 0) return 0;
  return (size_t)E * 3 * tiled_red_blocks(4LL * S * S) * 2 * sizeof(double);
}

int srpde_tiled_level_stats(const double* u_cur, const double* f_next, const double* theta_next, int E, int S,
                            float* stats, int* theta_const, void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_cur && f_next && theta_next && stats && theta_const && workspace,
                  "srpde_tiled_level_stats: null pointer");
  if (E <= 0 || S <= 0 || S > 16384 || E > 65535)
    TILED_FAIL(kErrShape, "srpde_tiled_level_stats: bad shape E=%d S=%d", E, S);
  if (reinterpret_cast<uintptr_t>(workspace) & 7u)
    TILED_FAIL(kErrAlign, "srpde_tiled_level_stats: workspace not 8-byte aligned");
  if (ws_bytes < srpde_tiled_level_stats_workspace_size(E, S))
    TILED_FAIL(kErrWorkspace, "srpde_tiled_level_stats: workspace too small");
  const long long n_u = (long long)S * S, n_f = 4 * n_u;
  const int nb_u = tiled_red_blocks(n_u), nb_f = tiled_red_blocks(n_f);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(tiled_stats_partial_kernel, dim3(nb_f, 3, E), dim3(kTiledRedThreads), 0, stream, u_cur, f_next,
                     theta_next, n_u, nb_u, n_f, part);
  SRPDE_LAUNCH_CHECK("srpde_tiled_level_stats");
  hipLaunchKernelGGL(tiled_stats_final_kernel, dim3(E), dim3(64), 0, stream, u_cur, f_next, theta_next, n_u, nb_u, n_f,
                     nb_f, part, stats, theta_const);
  SRPDE_LAUNCH_CHECK("srpde_tiled_level_stats");
  return 0;
}

int srpde_tiled_assemble(const double* u_cur, const double* f_next, const double* theta_next, const float* stats,
                         int E, int S, int tile, int stride, float* x, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_cur && f_next && theta_next && stats && x, "srpde_tiled_assemble: null pointer");
  TILED_CHECK_GEOMETRY("srpde_tiled_assemble");
  const long long total = (long long)E * m * m * (2 * tile) * (2 * tile);
  hipLaunchKernelGGL(tiled_assemble_kernel, dim3(tiled_grid(total)), dim3(256), 0, stream, u_cur, f_next, theta_next,
                     stats, E, S, tile, stride, m, x);
  SRPDE_LAUNCH_CHECK("srpde_tiled_assemble");
  return 0;
}

int srpde_tiled_blend_denorm(const float* y, const float* stats, int E, int S, int tile, int stride, int window,
                             double* u_next, hipStream_t stream) {
  SRPDE_CHECK_ARG(y && stats && u_next, "srpde_tiled_blend_denorm: null pointer");
  TILED_CHECK_GEOMETRY("srpde_tiled_blend_denorm");
  if (window != 0 && window != 1)
    TILED_FAIL(kErrArg, "srpde_tiled_blend_denorm: window=%d (0 = linear, 1 = flat)", window);
  const long long total = (long long)E * (2 * S) * (2 * S);
  if (window == 0)
    hipLaunchKernelGGL(tiled_blend_kernel<0>, dim3(tiled_grid(total)), dim3(256), 0, stream, y, stats, E, S, tile,
                       stride, m, u_next);
  else
    hipLaunchKernelGGL(tiled_blend_kernel<1>, dim3(tiled_grid(total)), dim3(256), 0, stream, y, stats, E, S, tile,
                       stride, m, u_next);
  SRPDE_LAUNCH_CHECK("srpde_tiled_blend_denorm");
  return 0;
}

}  // extern "C"
