// Batched cascade levels for E examples side by side (the repeated-example study of the reference's
// src/resolution_comparison_statistical.py over ml_multi_level_upscale, src/resolution_comparison.py:160-229), gfx950.
//
// One level of the cascade for E independent fields is four passes instead of ~20 torch launches and a host
// sync per example:
//   srpde_cascade_level_stats     GlobalNormalization's six statistics per example (+ the theta-constant flag,
//                                 decided on the device) from the next level's ground truth   [2 launches]
//   srpde_cascade_level_assemble  tile -> normalise -> bilinear x2 -> concat: the U-Net input  [1 launch]
//   srpde_cascade_stitch_denorm   U-Net output -> denormalise -> stitch -> fp64 field          [1 launch]
// and srpde_field_metrics gives MAE / RMSE / max error per example                             [2 launches].
//
// Tile order everywhere: example-major, then row-major over the (S / tile)^2 tiles of one example
// (resolution_comparison._blocks_to_tiles on [E, S, S] blocks).
//
// Reductions (statistics, metrics): every (example, field) is spread over red_blocks(n) workgroups, each
// grid-striding over its elements and leaving one fp64 partial per quantity; a second launch sums the partials
// in index order.  The element -> thread -> block assignment is a function of the shape alone, the in-block
// order is fixed (field_reduce.h: xor butterfly inside a wave, then the four waves in order), and there are no
// atomics, so the results are bit-reproducible from run to run.
//
// The statistics and assemble kernels serve tiled.hip too (cascade_level.h): the statistics take one length for u
// and one for f / theta, the assemble a window stride.  With equal lengths and stride == tile they are this
// file's disjoint-tile level; tiled.hip's is the same kernel, not a copy of it.
//
// Statistics are accumulated about the example's first value K (d = x - K, exact in fp64 for fp32-cast x):
// mean = K + sum(d) / n, var = (sum(d^2) - sum(d)^2 / n) / (n - 1).  The cancellation in var is then relative to
// (mean - K)^2 <= range^2, not to mean^2, so a nearly constant theta (std ~ 1e-6 around 1) keeps ~10 digits.
#include "cascade_level.h"
#include "common.h"
#include "field_reduce.h"
#include "resample.h"

namespace srpde {

// grid (red_blocks(n_f), 3 fields, E); field 0 = u (n_u values, nb_u workgroups; the others of its plane leave at
// once), fields 1 / 2 = f / theta (n_f values, every workgroup):
// part[((e * 3 + fld) * gridDim.x + b) * 2] = {sum d, sum d^2}, d = float(x) - float(x[0])
__global__ __launch_bounds__(kRedThreads) void level_stats_partial_kernel(const double* __restrict__ u,
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
  for (long long i = (long long)blockIdx.x * kRedThreads + threadIdx.x; i < n; i += (long long)nb * kRedThreads) {
    const double d = (double)(float)x[i] - K;
    s1 += d;
    s2 += d * d;
  }
  s1 = block_sum(s1, sh);
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) {
    double* p = part + (((long long)e * 3 + fld) * gridDim.x + blockIdx.x) * 2;
    p[0] = s1;
    p[1] = s2;
  }
}

// grid E, one wave: the partials of each field in index order -> the example's statistics row and theta flag
__global__ __launch_bounds__(64) void level_stats_final_kernel(const double* __restrict__ u,
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

// One thread per element of x [T][3][2 tile][2 tile]: channel 0 = bilinear x2 (align_corners, the expression of
// upsample_fwd_scalar_kernel) of the normalised coarse window, channel 1 = theta, channel 2 = f, normalised.  Each
// normalisation is an fp32 subtraction and a correctly rounded fp32 division, as the torch expressions.  Window k
// of the m per axis starts at min(k * stride, S - tile) on the coarse grid: k * tile for the disjoint tiles.
__global__ __launch_bounds__(256) void level_assemble_kernel(const double* __restrict__ u_cur,
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
    const int sy = min(ti * stride, S - tile), sx = min(tj * stride, S - tile);
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
    // ly.l0 * (lx.l0 * a + lx.l1 * b) + ly.l1 * (lx.l0 * d + lx.l1 * f) with the contraction the compiler makes of
    // it in upsample_fwd_scalar_kernel spelt out (one product rounded, the other fused, three times): left to
    // itself it fuses the other product here, where the taps come out of divisions, and results move by an ulp
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

// One thread per element of u_next [E][2S][2S]: y * u_std + u_mean as an fp32 multiply, then an fp32 add (two
// roundings, as torch's y * std + mean), widened to fp64, from the tile that holds the pixel.
__global__ __launch_bounds__(256) void cascade_stitch_kernel(const float* __restrict__ yt,
                                                             const float* __restrict__ stats, int E, int S, int tile,
                                                             double* __restrict__ u_next) {
  const int m = S / tile, t2 = 2 * tile, S2 = 2 * S;
  const long long field = (long long)S2 * S2, total = (long long)E * field;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(q / field);
    const int pix = (int)(q - (long long)e * field), Y = pix / S2, X = pix - Y * S2;
    const int ti = Y / t2, y = Y - ti * t2, tj = X / t2, x = X - tj * t2;
    const float v = yt[(((long long)e * m + ti) * m + tj) * t2 * t2 + y * t2 + x];
    u_next[q] = (double)denorm(v, stats[e * 6 + 1], stats[e * 6]);
  }
}

// grid (red_blocks, E): part[(e * nb + b) * 3] = {sum |d|, sum d^2, max |d|}, d = pred - gt in fp64
template <typename TP>
__global__ __launch_bounds__(kRedThreads) void field_metrics_partial_kernel(const TP* __restrict__ pred,
                                                                            const double* __restrict__ gt,
                                                                            long long n, double* __restrict__ part) {
  __shared__ double sh[4];
  const int e = blockIdx.y;
  const TP* p = pred + (long long)e * n;
  const double* g = gt + (long long)e * n;
  double sa = 0.0, sq = 0.0, mx = 0.0;
  for (long long i = (long long)blockIdx.x * kRedThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kRedThreads) {
    const double d = (double)p[i] - g[i];
    sa += fabs(d);
    sq += d * d;
    mx = fmax(mx, fabs(d));
  }
  sa = block_sum(sa, sh);
  sq = block_sum(sq, sh);
  block_max_store(mx, sh);
  if (threadIdx.x == 0) {
    double* o = part + ((long long)e * gridDim.x + blockIdx.x) * 3;
    o[0] = sa;
    o[1] = sq;
    o[2] = block_max_load(sh);
  }
}

__global__ __launch_bounds__(64) void field_metrics_final_kernel(const double* __restrict__ part, int nb, long long n,
                                                                 double* __restrict__ out) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const double* p = part + (long long)e * nb * 3;
  double sa = 0.0, sq = 0.0, mx = 0.0;
  for (int j = lane; j < nb; j += 64) {
    sa += p[3 * j];
    sq += p[3 * j + 1];
    mx = fmax(mx, p[3 * j + 2]);
  }
  sa = wave_sum(sa);
  sq = wave_sum(sq);
  mx = wave_max(mx);
  if (lane == 0) {
    out[e * 3] = sa / (double)n;
    out[e * 3 + 1] = sqrt(sq / (double)n);
    out[e * 3 + 2] = mx;
  }
}

int level_stats_launch(const char* name, const double* u, const double* f, const double* th, long long n_u,
                       long long n_f, int E, float* stats, int* theta_const, double* part, hipStream_t stream) {
  const int nb_u = red_blocks(n_u), nb_f = red_blocks(n_f);
  hipLaunchKernelGGL(level_stats_partial_kernel, dim3(nb_f, 3, E), dim3(kRedThreads), 0, stream, u, f, th, n_u, nb_u,
                     n_f, part);
  SRPDE_LAUNCH_CHECK(name);
  hipLaunchKernelGGL(level_stats_final_kernel, dim3(E), dim3(64), 0, stream, u, f, th, n_u, nb_u, n_f, nb_f, part, stats,
                     theta_const);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int level_assemble_launch(const char* name, const double* u_cur, const double* f_next, const double* th_next,
                          const float* stats, int E, int S, int tile, int stride, int m, float* x, hipStream_t stream) {
  const long long total = (long long)E * m * m * (2 * tile) * (2 * tile);
  hipLaunchKernelGGL(level_assemble_kernel, dim3(elementwise_grid(total)), dim3(256), 0, stream, u_cur, f_next, th_next,
                     stats, E, S, tile, stride, m, x);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace srpde

using namespace srpde;

extern "C" {

size_t srpde_cascade_level_stats_workspace_size(int E, int S2) {
  if (E <= 0 || S2 <= 0) return 0;
  return (size_t)E * 3 * red_blocks((long long)S2 * S2) * 2 * sizeof(double);
}

int srpde_cascade_level_stats(const double* u, const double* f, const double* theta, int E, int S2, float* stats,
                              int* theta_const, void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(u && f && theta && stats && theta_const && workspace, "srpde_cascade_level_stats: null pointer");
  if (E <= 0 || S2 <= 0 || E > 65535) SRPDE_FAIL(kErrShape, "srpde_cascade_level_stats: bad shape E=%d S2=%d", E, S2);
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) SRPDE_FAIL(kErrAlign, "srpde_cascade_level_stats: workspace not 8-byte aligned");
  if (ws_bytes < srpde_cascade_level_stats_workspace_size(E, S2))
    SRPDE_FAIL(kErrWorkspace, "srpde_cascade_level_stats: workspace too small");
  const long long n = (long long)S2 * S2;
  return level_stats_launch("srpde_cascade_level_stats", u, f, theta, n, n, E, stats, theta_const,
                            static_cast<double*>(workspace), stream);
}

int srpde_cascade_level_assemble(const double* u_cur, const double* f_next, const double* theta_next,
                                 const float* stats, int E, int S, int tile, float* x, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_cur && f_next && theta_next && stats && x, "srpde_cascade_level_assemble: null pointer");
  if (E <= 0 || S <= 0 || tile <= 0 || S % tile != 0 || S > 16384)
    SRPDE_FAIL(kErrShape, "srpde_cascade_level_assemble: bad shape E=%d S=%d tile=%d (S must be a multiple of tile)", E,
               S, tile);
  return level_assemble_launch("srpde_cascade_level_assemble", u_cur, f_next, theta_next, stats, E, S, tile, tile,
                               S / tile, x, stream);
}

int srpde_cascade_stitch_denorm(const float* y, const float* stats, int E, int S, int tile, double* u_next,
                                hipStream_t stream) {
  SRPDE_CHECK_ARG(y && stats && u_next, "srpde_cascade_stitch_denorm: null pointer");
  if (E <= 0 || S <= 0 || tile <= 0 || S % tile != 0 || S > 16384)
    SRPDE_FAIL(kErrShape, "srpde_cascade_stitch_denorm: bad shape E=%d S=%d tile=%d (S must be a multiple of tile)", E,
               S, tile);
  const long long total = (long long)E * (2 * S) * (2 * S);
  hipLaunchKernelGGL(cascade_stitch_kernel, dim3(elementwise_grid(total)), dim3(256), 0, stream, y, stats, E, S, tile,
                     u_next);
  SRPDE_LAUNCH_CHECK("srpde_cascade_stitch_denorm");
  return 0;
}

size_t srpde_field_metrics_workspace_size(int E, int n) {
  if (E <= 0 || n <= 0) return 0;
  return (size_t)E * red_blocks((long long)n * n) * 3 * sizeof(double);
}

int srpde_field_metrics(const void* pred, int pred_is_f32, const double* gt, int E, int n, double* out,
                        void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(pred && gt && out && workspace, "srpde_field_metrics: null pointer");
  if (E <= 0 || n <= 0 || E > 65535) SRPDE_FAIL(kErrShape, "srpde_field_metrics: bad shape E=%d n=%d", E, n);
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) SRPDE_FAIL(kErrAlign, "srpde_field_metrics: workspace not 8-byte aligned");
  if (ws_bytes < srpde_field_metrics_workspace_size(E, n))
    SRPDE_FAIL(kErrWorkspace, "srpde_field_metrics: workspace too small");
  const long long nn = (long long)n * n;
  const int nb = red_blocks(nn);
  double* part = static_cast<double*>(workspace);
  if (pred_is_f32)
    hipLaunchKernelGGL(field_metrics_partial_kernel<float>, dim3(nb, E), dim3(kRedThreads), 0, stream,
                       static_cast<const float*>(pred), gt, nn, part);
  else
    hipLaunchKernelGGL(field_metrics_partial_kernel<double>, dim3(nb, E), dim3(kRedThreads), 0, stream,
                       static_cast<const double*>(pred), gt, nn, part);
  SRPDE_LAUNCH_CHECK("srpde_field_metrics");
  hipLaunchKernelGGL(field_metrics_final_kernel, dim3(E), dim3(64), 0, stream, part, nb, nn, out);
  SRPDE_LAUNCH_CHECK("srpde_field_metrics");
  return 0;
}

}  // extern "C"
