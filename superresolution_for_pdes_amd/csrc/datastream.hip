// Device-side sample generator for streamed training batches (online.SampleStream), gfx950.
//
// A training sample of the reference's dataset is a handful of random scalars (two wave numbers, for a subdomain
// sample also a crop start) and, optionally, a random coefficient field theta.  Here they come from a counter-based
// generator, so a batch needs no host draw and no host copy: seed, first sample index and sizes travel as kernel
// arguments, and
//   srpde_stream_draw    writes k12, starts and theta for B consecutive samples        [1 launch]
//   srpde_stream_window  crops / strides the solved fp64 fields into the fp32 training fields  [1 launch]
//   srpde_stream_walls   writes smooth random boundary data for B consecutive samples           [1 launch]
// with srpde_forcing_batched, the Poisson solvers and srpde_pde_dataset_assemble in between.
//
// Generator: Philox4x32-10 (Salmon et al., SC'11), a pure function of (seed, sample, field, element):
//   key     = (seed low word, seed high word)
//   counter = (element, field, sample low word, sample high word)
// so a sample's values do not depend on the batch size, the rank count or the launch geometry.  A uniform double
// comes from an ordered pair of output words (a, b): u = (((uint64)a << 32 | b) >> 11) * 2^-53, in [0, 1).
//   field 0 (scalars): element 0 -> k1 (words 0,1), k2 (words 2,3); element 1 -> start_x (0,1), start_y (2,3)
//   field 1 (theta)  : element e -> pixels 2e (words 0,1) and 2e + 1 (words 2,3) of the row-major [n][n] grid
//   field 2 (walls)  : element e = 0 .. 7 -> side e >> 1 (row 0, row n - 1, column 0, column n - 1), the coefficients of
//                      its cosine modes m = 2 (e & 1) (words 0,1) and m + 1 (words 2,3): c = (amp * (2 u - 1)) / (m + 1)
// A value in a range is lo + (hi - lo) * u as a rounded product, then a rounded sum (contraction off), a start is
// (int)floor(u * max_start): both are what numpy computes from the same u, bit for bit.  u * max_start never
// rounds up to max_start (max_start * 2^-53 is at least half an ulp below it), so the upper bound is exclusive.
#include "common.h"
#include "field_reduce.h"

namespace srpde {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr int kFieldScalars = 0, kFieldTheta = 1, kFieldWalls = 2;

struct Words4 {
  uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ Words4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return {c0, c1, c2, c3};
}

__device__ __forceinline__ Words4 stream_words(long long seed, long long sample, uint32_t field, uint32_t element) {
  const unsigned long long s = (unsigned long long)seed, i = (unsigned long long)sample;
  return philox4x32_10(element, field, (uint32_t)i, (uint32_t)(i >> 32), (uint32_t)s, (uint32_t)(s >> 32));
}

__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {
  return (double)((((unsigned long long)a << 32) | b) >> 11) * 0x1p-53;
}

__device__ __forceinline__ double in_range(double lo, double hi, double u) {
#pragma clang fp contract(off)
  const double t = (hi - lo) * u;
  return lo + t;
}

// out[(s * ne + e) * 4 ..] = the four words of (seed, sample0 + s, field, element0 + e)
__global__ __launch_bounds__(256) void stream_raw_kernel(long long seed, long long sample0, long long ns, uint32_t field,
                                                         uint32_t element0, long long ne, uint32_t* __restrict__ out) {
  const long long total = ns * ne;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const long long s = q / ne, e = q - s * ne;
    // (the sample index wraps in two's complement, like the counter words it fills)
    const long long sample = (long long)((unsigned long long)sample0 + (unsigned long long)s);
    const Words4 w = stream_words(seed, sample, field, element0 + (uint32_t)e);
    uint32_t* o = out + q * 4;
    o[0] = w.w0;
    o[1] = w.w1;
    o[2] = w.w2;
    o[3] = w.w3;
  }
}

// One thread per (sample, slot): slots 0 .. ne - 1 are the theta elements (two pixels each, ne = ceil(n^2 / 2), 0
// without a theta output), slot ne the sample's scalars.  theta_half (nullable) is theta[::2, ::2].
__global__ __launch_bounds__(256) void stream_draw_kernel(long long seed, long long sample0, int B, double k_lo,
                                                          double k_hi, int theta_uniform, double th_lo, double th_hi,
                                                          int n, int max_start, double* __restrict__ k12,
                                                          int* __restrict__ starts, double* __restrict__ theta,
                                                          double* __restrict__ theta_half) {
  const long long n2 = theta ? (long long)n * n : 0, ne = (n2 + 1) / 2, slots = ne + 1, total = (long long)B * slots;
  const int nh = (n + 1) / 2;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const long long b = q / slots, e = q - b * slots;
    const long long sample = (long long)((unsigned long long)sample0 + (unsigned long long)b);
    if (e == ne) {
      const Words4 w = stream_words(seed, sample, kFieldScalars, 0);
      k12[2 * b] = in_range(k_lo, k_hi, uniform53(w.w0, w.w1));
      k12[2 * b + 1] = in_range(k_lo, k_hi, uniform53(w.w2, w.w3));
      if (starts) {
        const Words4 v = stream_words(seed, sample, kFieldScalars, 1);
        starts[2 * b] = (int)floor(uniform53(v.w0, v.w1) * (double)max_start);
        starts[2 * b + 1] = (int)floor(uniform53(v.w2, v.w3) * (double)max_start);
      }
      continue;
    }
    double v0 = 1.0, v1 = 1.0;
    if (theta_uniform) {
      const Words4 w = stream_words(seed, sample, kFieldTheta, (uint32_t)e);
      v0 = in_range(th_lo, th_hi, uniform53(w.w0, w.w1));
      v1 = in_range(th_lo, th_hi, uniform53(w.w2, w.w3));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long p = 2 * e + j;
      if (p >= n2) break;
      const double v = j ? v1 : v0;
      theta[b * n2 + p] = v;
      if (theta_half) {
        const int r = (int)(p / n), c = (int)(p - (long long)r * n);
        if (!((r | c) & 1)) theta_half[(b * nh + (r >> 1)) * nh + (c >> 1)] = v;
      }
    }
  }
}

// One thread per pixel of the [B][nf][nf] window: the three fine fields cast to fp32, and from the pixels with even
// row and column the stride-2 coarse field.  starts == nullptr: the window is the whole field (ns == nf) and the
// coarse field is the cast of coarse_in [B][nc][nc], a solve of its own.  A start outside [0, ns - nf] is clamped,
// so no start value read from memory can take an access out of the fields.
__global__ __launch_bounds__(256) void stream_window_kernel(const double* __restrict__ u, const double* __restrict__ f,
                                                            const double* __restrict__ th,
                                                            const int* __restrict__ starts,
                                                            const double* __restrict__ coarse_in, int B, int ns, int nf,
                                                            float* __restrict__ u_fine, float* __restrict__ f_fine,
                                                            float* __restrict__ th_fine, float* __restrict__ u_coarse) {
  const int nc = (nf + 1) / 2;
  const long long plane = (long long)nf * nf, total = (long long)B * plane, field = (long long)ns * ns;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const long long b = q / plane;
    const int pix = (int)(q - b * plane), i = pix / nf, j = pix - i * nf;
    int sx = 0, sy = 0;
    if (starts) {
      sx = min(max(starts[2 * b], 0), ns - nf);
      sy = min(max(starts[2 * b + 1], 0), ns - nf);
    }
    const long long src = b * field + (long long)(sy + i) * ns + (sx + j);
    const float uv = (float)u[src];
    u_fine[q] = uv;
    f_fine[q] = (float)f[src];
    th_fine[q] = (float)th[src];
    if (!((i | j) & 1)) {
      const long long c = (b * nc + (i >> 1)) * nc + (j >> 1);
      u_coarse[c] = coarse_in ? (float)coarse_in[c] : uv;
    }
  }
}

// c = (amp * (2 u - 1)) / (m + 1): 2 u - 1 is exact, the product and the quotient are rounded once each
__device__ __forceinline__ double wall_coef(double amp, double u, int m) {
#pragma clang fp contract(off)
  const double v = 2.0 * u - 1.0;
  const double t = amp * v;
  return t / (double)(m + 1);
}

// cos(pi m k / (n - 1)), the argument reduced in integers
__device__ __forceinline__ double wall_cos(int m, int k, int n1) { return cospi((double)((m * k) % (2 * n1)) / (double)n1); }

// One thread per entry (sample, side, k) of bd [B][4][n]: the side's four coefficients from its two field-2 elements,
// then (c0 cos(0) + c1 cos(pi k / (n - 1))) + (c2 cos(2 pi k / (n - 1)) + c3 cos(3 pi k / (n - 1))).  An even k also
// writes entry k / 2 of bd_half [B][4][(n + 1) / 2] (nullable); bd_f32 (nullable) is the fp32 cast.
__global__ __launch_bounds__(256) void stream_walls_kernel(long long seed, long long sample0, int B, int n, int bc,
                                                           double g_amp, double q_amp, double* __restrict__ bd,
                                                           double* __restrict__ bd_half, float* __restrict__ bd_f32) {
#pragma clang fp contract(off)
  const long long total = (long long)B * 4 * n;
  const int nh = (n + 1) / 2, n1 = n - 1;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const long long row = q / n, b = row >> 2;
    const int k = (int)(q - row * n), side = (int)(row & 3);
    const long long sample = (long long)((unsigned long long)sample0 + (unsigned long long)b);
    const double amp = (bc >> side) & 1 ? q_amp : g_amp;
    const Words4 lo = stream_words(seed, sample, kFieldWalls, 2 * side);
    const Words4 hi = stream_words(seed, sample, kFieldWalls, 2 * side + 1);
    const double c0 = wall_coef(amp, uniform53(lo.w0, lo.w1), 0), c1 = wall_coef(amp, uniform53(lo.w2, lo.w3), 1);
    const double c2 = wall_coef(amp, uniform53(hi.w0, hi.w1), 2), c3 = wall_coef(amp, uniform53(hi.w2, hi.w3), 3);
    const double t0 = c0 * wall_cos(0, k, n1), t1 = c1 * wall_cos(1, k, n1);
    const double t2 = c2 * wall_cos(2, k, n1), t3 = c3 * wall_cos(3, k, n1);
    const double v = (t0 + t1) + (t2 + t3);
    bd[q] = v;
    if (bd_f32) bd_f32[q] = (float)v;
    if (bd_half && !(k & 1)) bd_half[row * nh + (k >> 1)] = v;
  }
}

}  // namespace srpde

using namespace srpde;

extern "C" {

int srpde_stream_raw(long long seed, long long sample0, long long n_samples, long long field, long long element0,
                     long long n_elements, unsigned* out, hipStream_t stream) {
  SRPDE_CHECK_ARG(out, "srpde_stream_raw: null pointer");
  if (n_samples <= 0 || n_elements <= 0 || n_samples > (1LL << 31) / n_elements)
    SRPDE_FAIL(kErrShape, "srpde_stream_raw: bad counts n_samples=%lld n_elements=%lld (product up to 2^31)", n_samples,
               n_elements);
  if (field < 0 || field > 0xffffffffLL || element0 < 0 || element0 + n_elements > (1LL << 32))
    SRPDE_FAIL(kErrArg, "srpde_stream_raw: field %lld / elements %lld + %lld outside a 32-bit counter word", field,
               element0, n_elements);
  hipLaunchKernelGGL(stream_raw_kernel, dim3(elementwise_grid(n_samples * n_elements)), dim3(256), 0, stream, seed,
                     sample0, n_samples, (uint32_t)field, (uint32_t)element0, n_elements, out);
  SRPDE_LAUNCH_CHECK("srpde_stream_raw");
  return 0;
}

int srpde_stream_draw(long long seed, long long sample0, int B, double k_lo, double k_hi, int theta_mode,
                      double theta_lo, double theta_hi, int n, int max_start, double* k12, int* starts, double* theta,
                      double* theta_half, hipStream_t stream) {
  SRPDE_CHECK_ARG(k12, "srpde_stream_draw: null k12");
  SRPDE_CHECK_ARG(theta || !theta_half, "srpde_stream_draw: theta_half without theta");
  if (B <= 0) SRPDE_FAIL(kErrShape, "srpde_stream_draw: bad B=%d", B);
  if (theta_mode != 0 && theta_mode != 1)
    SRPDE_FAIL(kErrArg, "srpde_stream_draw: theta_mode %d (0: ones, 1: uniform)", theta_mode);
  if (theta && (n < 1 || n > 16384)) SRPDE_FAIL(kErrShape, "srpde_stream_draw: bad n=%d", n);
  if (starts && max_start < 1) SRPDE_FAIL(kErrArg, "srpde_stream_draw: max_start %d < 1", max_start);
  if (!(k_lo <= k_hi) || (theta && theta_mode == 1 && !(theta_lo <= theta_hi)))
    SRPDE_FAIL(kErrArg, "srpde_stream_draw: empty range k [%g, %g] theta [%g, %g]", k_lo, k_hi, theta_lo, theta_hi);
  const long long n2 = theta ? (long long)n * n : 0;
  hipLaunchKernelGGL(stream_draw_kernel, dim3(elementwise_grid((long long)B * ((n2 + 1) / 2 + 1))), dim3(256), 0,
                     stream, seed, sample0, B, k_lo, k_hi, theta_mode, theta_lo, theta_hi, n, max_start, k12, starts,
                     theta, theta_half);
  SRPDE_LAUNCH_CHECK("srpde_stream_draw");
  return 0;
}

int srpde_stream_walls(long long seed, long long sample0, int B, int n, int bc, double g_amp, double q_amp, double* bd,
                       double* bd_half, float* bd_f32, hipStream_t stream) {
  SRPDE_CHECK_ARG(bd, "srpde_stream_walls: null bd");
  if (B <= 0 || n < 2 || n > 16384) SRPDE_FAIL(kErrShape, "srpde_stream_walls: bad shape B=%d n=%d (n >= 2)", B, n);
  if (bc < 0 || bc > 15)
    SRPDE_FAIL(kErrArg, "srpde_stream_walls: bc=%d is not a side mask (bits 0..3: row 0, row n-1, column 0, column n-1)",
               bc);
  if (!(g_amp == g_amp) || !(q_amp == q_amp) || g_amp - g_amp != 0.0 || q_amp - q_amp != 0.0)
    SRPDE_FAIL(kErrArg, "srpde_stream_walls: amplitudes g_amp=%g q_amp=%g are not finite", g_amp, q_amp);
  hipLaunchKernelGGL(stream_walls_kernel, dim3(elementwise_grid((long long)B * 4 * n)), dim3(256), 0, stream, seed,
                     sample0, B, n, bc, g_amp, q_amp, bd, bd_half, bd_f32);
  SRPDE_LAUNCH_CHECK("srpde_stream_walls");
  return 0;
}

int srpde_stream_window(const double* u, const double* f, const double* theta, const int* starts,
                        const double* u_coarse_in, int B, int ns, int nf, float* u_fine, float* f_fine,
                        float* theta_fine, float* u_coarse, hipStream_t stream) {
  SRPDE_CHECK_ARG(u && f && theta && u_fine && f_fine && theta_fine && u_coarse, "srpde_stream_window: null pointer");
  if (B <= 0 || nf < 1 || ns < nf || ns > 16384)
    SRPDE_FAIL(kErrShape, "srpde_stream_window: bad shape B=%d ns=%d nf=%d", B, ns, nf);
  if (!starts && ns != nf)
    SRPDE_FAIL(kErrShape, "srpde_stream_window: without starts the window is the field (ns=%d, nf=%d)", ns, nf);
  if (starts && u_coarse_in)
    SRPDE_FAIL(kErrArg, "srpde_stream_window: u_coarse_in belongs to the pass-through variant (starts == NULL)");
  hipLaunchKernelGGL(stream_window_kernel, dim3(elementwise_grid((long long)B * nf * nf)), dim3(256), 0, stream, u, f,
                     theta, starts, u_coarse_in, B, ns, nf, u_fine, f_fine, theta_fine, u_coarse);
  SRPDE_LAUNCH_CHECK("srpde_stream_window");
  return 0;
}

}  // extern "C"
