// Direct Poisson solve by the 2-D sine transform (DST-I), gfx950, fp64 MFMA.
//
// The operator of srpde_poisson_cg_batched, theta * L u = f with L the 5-point Laplacian on all n^2 nodes of an
// n x n grid (zero ghost ring, h = 1 / (n - 1)), is L = (T (x) I + I (x) T) / h^2 with T = tridiag(1, -2, 1).
// The symmetric orthogonal sine matrix S[j][k] = sqrt(2 / (n + 1)) sin(pi (j + 1)(k + 1) / (n + 1)) diagonalises
// T with eigenvalues lam_k = -4 sin^2(pi (k + 1) / (2 (n + 1))), hence exactly
//
//     U = S ( (S (F / Theta) S) o h^2 / (lam_i + lam_j) ) S
//
// four dense n x n products per problem against one fixed matrix: no iteration, no convergence test, no
// cooperative launch, no grid barrier.
//
//   srpde_poisson_dst_plan     fills the caller-owned plan: S [n][n] then lam [n] (the library keeps no state).
//                              The sine argument is reduced in integers, m = (j + 1)(k + 1) mod 2 (n + 1), and
//                              evaluated as sinpi(m / (n + 1)): sin(pi j k / (n + 1)) loses ~1e-13 at n = 640.
//   n <= kDstLdsMaxN           dst_fused_kernel: one workgroup per problem, S and the field in LDS (zero-padded
//                              to whole 16 x 16 tiles), every product accumulated in registers and written back
//                              after a barrier; f and theta are read once, u is written once.  One launch.
//   any other n                dst_gemm_kernel: a batched 64 x 64-tile product C[b] = A[b] B[b] where either
//                              operand may be the shared S (batch stride 0): X S, then S X, X S, S X.  The
//                              division by theta is in the first product's operand load, the multiplication by
//                              h^2 / (lam_i + lam_j) in the second product's store.  Four launches.
//
// Both use v_mfma_f64_16x16x4_f64.  Lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] and
// holds C[row (l >> 4) + 4 r][col l & 15] in register r = 0..3 (not the f32 16x16 map).
//
// Shifted solve (srpde_poisson_dst_shift_batched, the preconditioner of the shifted CG of poisson_div.hip): S
// diagonalises L - sigma I as well, with eigenvalues (lam_i + lam_j) / h^2 - sigma, so the same products solve
// (L - sigma I) u = f once the scaling h^2 / (lam_i + lam_j) becomes dst_shift_scale's 1 / ((lam_i + lam_j) inv_h2 -
// sigma).  It is a template argument of the two kernels that scale; sigma = 0 launches the unshifted instantiations.
//
// Separable solve with mixed sides (srpde_poisson_sep_*, the preconditioner of the *_bc CG of poisson_div.hip).  A side
// of the grid is the zero ghost ring (Dirichlet) or zero flux (Neumann: the ghost face is missing), given as the 4-bit
// mask bc of poisson_div.hip.  The constant-coefficient operator is still L_bc = (T_y (x) I + I (x) T_x) / h^2, each T
// tridiagonal with 1 off the diagonal and -2 on it, -1 at a Neumann end; its orthogonal eigenvector matrices Q_y, Q_x
// (sine, quarter-wave sine or cosine: sep_axis_kernel) are no longer symmetric and differ per axis, so the plan holds
// each with its transpose and
//     U = Q_y ( (Q_y^T F Q_x) o 1 / ((lam_y,i + lam_x,j) inv_h2 - sigma_p) ) Q_x^T
// is the four launches of dst_gemm_kernel of the general path at every n (SCALE 3: dst_shift_scale with the row's
// eigenvalue from lam_y and the column's from lam_x).  The one-workgroup LDS kernel is not extended.
//
// The k order of every sum is ascending and fixed by n alone, there are no atomics, and a problem's blocks
// never see another problem: results are bit-reproducible and independent of B.
#include <cmath>

#include "common.h"
#include "field_reduce.h"
#include "poisson_dst.h"

namespace srpde {

using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int kDstLdsMaxN = 96;     // two [96][98] fp64 buffers: 150,528 of the CU's 163,840 bytes of LDS
constexpr int kDstMaxN = 16384;     // n^2 stays inside int

static size_t dst_plan_bytes(int n) { return ((size_t)n * n + (size_t)n) * sizeof(double); }

__device__ __forceinline__ d4 mfma_f64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void dst_plan_kernel(int n, double* __restrict__ S, double* __restrict__ lam) {
  const long long total = (long long)n * n;
  const int n1 = n + 1;
  const double scale = sqrt(2.0 / (double)n1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i / n), k = (int)(i - (long long)j * n);
    const long long m = ((long long)(j + 1) * (k + 1)) % (2LL * n1);
    S[i] = scale * sinpi((double)m / (double)n1);
    if (i < n) {
      const double s = sinpi((double)(i + 1) / (2.0 * (double)n1));
      lam[i] = -4.0 * s * s;
    }
  }
}

// The shifted eigenvalue scaling, every operation rounded once in this order (no contraction): the sum lam_i + lam_j,
// times inv_h2 = (n - 1)^2, minus sigma, then the reciprocal.  sigma >= 0 and the sum is negative: never 0.
__device__ __forceinline__ double dst_shift_scale(double li, double lj, double inv_h2, double sigma) {
#pragma clang fp contract(off)
  const double s = li + lj;
  const double d = s * inv_h2;
  return 1.0 / (d - sigma);
}

// One axis of the separable plan.  Nodes j = 0 .. n - 1, modes k = 0 .. n - 1, column k of Q the unit eigenvector:
//   Dirichlet both ends (nlo = nhi = 0)   sqrt(2 / (n + 1)) sin(pi (j + 1)(k + 1) / (n + 1)),    s = (k + 1) / (2 (n + 1))
//   Dirichlet at 0, Neumann at n - 1      (2 / sqrt(2 n + 1)) sin(pi (j + 1)(2 k + 1) / (2 n + 1)), s = (2 k + 1) / (2 (2 n + 1))
//   Neumann at 0, Dirichlet at n - 1      the same with j -> n - 1 - j
//   Neumann both ends                     sqrt((k ? 2 : 1) / n) cos(pi (2 j + 1) k / (2 n)),      s = k / (2 n)
// and lam_k = -4 sin^2(pi s).  The arguments are reduced in integers before sinpi, as dst_plan_kernel does;
// cos(pi m / (2 n)) is taken as sin(pi (m + n) / (2 n)), still in integers, so every entry is one sinpi of a quotient
// of two integers.
__global__ __launch_bounds__(256) void sep_axis_kernel(int n, int nlo, int nhi, double* __restrict__ Q,
                                                       double* __restrict__ QT, double* __restrict__ lam,
                                                       double* __restrict__ mask_word, int bc) {
  const long long total = (long long)n * n;
  const bool dd = !nlo && !nhi, nn = nlo && nhi;
  const int den = dd ? n + 1 : (nn ? 2 * n : 2 * n + 1);          // the entries' sinpi(m / den), m mod 2 den
  const int lden = dd ? n + 1 : (nn ? n : 2 * n + 1);             // the eigenvalues' sinpi(num / (2 lden))
  const double scale = dd ? sqrt(2.0 / (double)(n + 1)) : (nn ? sqrt(2.0 / (double)n) : 2.0 / sqrt((double)(2 * n + 1)));
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i / n), k = (int)(i - (long long)j * n);
    const int jj = (!nn && nlo) ? n - 1 - j : j;
    long long m;
    if (dd)
      m = (long long)(jj + 1) * (k + 1);
    else if (nn)
      m = (long long)(2 * jj + 1) * k + n;
    else
      m = (long long)(jj + 1) * (2 * k + 1);
    m %= 2LL * den;
    double q = scale * sinpi((double)m / (double)den);
    if (nn && k == 0) q = sqrt(1.0 / (double)n);                  // the constant mode
    Q[i] = q;
    QT[(long long)k * n + j] = q;
    if (i < n) {
      const int num = dd ? (int)i + 1 : (nn ? (int)i : 2 * (int)i + 1);
      const double sv = sinpi((double)num / (2.0 * (double)lden));
      lam[i] = -4.0 * sv * sv;
    }
    if (i == 0 && mask_word) *mask_word = (double)bc;
  }
}

// the mask word, then mask more words: a plan is tied to its n AND its mask by its size (the entries see only the
// device pointer and the size, and read nothing back)
static size_t sep_plan_bytes(int n, int bc) {
  return ((size_t)4 * n * n + (size_t)2 * n + 1 + (size_t)bc) * sizeof(double);
}

// ---- general path ------------------------------------------------------------------------------------------
constexpr int kGT = 64;            // block tile (rows and columns); four waves, 32 x 32 each
constexpr int kGK = 16;            // k per LDS stage
constexpr int kGLdA = kGK + 1;     // As[m][k]: lanes 0..15 read 16 rows at one k, 17 spreads them over the banks
constexpr int kGLdB = kGT + 16;    // Bs[k][c]: the two k rows of a half wave land 32 banks apart

// C[b] = A[b] B[b], all [n][n] row-major, batch strides sA / sB / sC in elements (0: shared by every problem).
// DIV: A's elements are divided by th's (same indexing as A) as they are loaded.
// SCALE 1: C[i][j] is multiplied by h2 / (lam[i] + lam[j]) as it is stored; SCALE 2: by dst_shift_scale(lam[i],
// lam[j], inv_h2, sigma) instead; SCALE 3: by dst_shift_scale(lam[i], lam[n + j], inv_h2, sigma), the row's eigenvalue
// from the first and the column's from the second of two vectors [n] (the separable solve's lam_y, lam_x).
template <bool DIV, int SCALE>
__global__ __launch_bounds__(256) void dst_gemm_kernel(const double* __restrict__ A, long long sA,
                                                       const double* __restrict__ Bm, long long sB,
                                                       double* __restrict__ C, long long sC,
                                                       const double* __restrict__ th, const double* __restrict__ lam,
                                                       double h2, double inv_h2, double sigma, int n,
                                                       int nbatch) {
  __shared__ double As[kGT * kGLdA];
  __shared__ double Bs[kGK * kGLdB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int m0 = blockIdx.y * kGT, c0 = blockIdx.x * kGT;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int ka = tid & 15, ma = tid >> 4;   // A stage: rows ma + 16 i, column ka
  const int cb = tid & 63, kb = tid >> 6;   // B stage: rows kb + 4 i, column cb

  for (int b = blockIdx.z; b < nbatch; b += gridDim.z) {
    const double* Ab = A + (long long)b * sA;
    const double* Tb = DIV ? th + (long long)b * sA : nullptr;
    const double* Bb = Bm + (long long)b * sB;
    double* Cb = C + (long long)b * sC;
    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    double ra[4], rb[4];

    auto fetch = [&](int k0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = m0 + ma + 16 * i, c = k0 + ka;
        double v = 0.0;
        if (r < n && c < n) {
          const long long at = (long long)r * n + c;
          v = Ab[at];
          if (DIV) v = v / Tb[at];
        }
        ra[i] = v;
        const int rk = k0 + kb + 4 * i, cc = c0 + cb;
        rb[i] = (rk < n && cc < n) ? Bb[(long long)rk * n + cc] : 0.0;
      }
    };

    fetch(0);
    for (int k0 = 0; k0 < n; k0 += kGK) {
      __syncthreads();   // the previous stage's reads are over
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        As[(ma + 16 * i) * kGLdA + ka] = ra[i];
        Bs[(kb + 4 * i) * kGLdB + cb] = rb[i];
      }
      __syncthreads();
      if (k0 + kGK < n) fetch(k0 + kGK);
#pragma unroll
      for (int ks = 0; ks < kGK / 4; ++ks) {
        const int k = 4 * ks + l4;
        const double a0 = As[(wr + l15) * kGLdA + k], a1 = As[(wr + 16 + l15) * kGLdA + k];
        const double b0 = Bs[k * kGLdB + wc + l15], b1 = Bs[k * kGLdB + wc + 16 + l15];
        acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
        acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
        acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
        acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = c0 + wc + 16 * j + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wr + 16 * i + l4 + 4 * r;
          if (row < n && col < n) {
            double v = acc[i][j][r];
            if (SCALE == 1) v = v * (h2 / (lam[row] + lam[col]));
            if (SCALE == 2) v = v * dst_shift_scale(lam[row], lam[col], inv_h2, sigma);
            if (SCALE == 3) v = v * dst_shift_scale(lam[row], lam[n + col], inv_h2, sigma);
            Cb[(long long)row * n + col] = v;
          }
        }
      }
  }
}

// ---- fused small-n path ------------------------------------------------------------------------------------
// One workgroup per problem; np = n rounded up to 16, ld = np + 2, LDS = Sl[np][ld] then Xl[np][ld], both
// zero outside [n][n] so no product needs an edge guard.  The np / 16 row strips of a product are split into
// column groups of at most three 16 x 16 tiles; each wave owns one (strip, group) -- the launch has exactly
// that many waves (at most 12).  Products alternate X S (even) and S X (odd; S's fragment is read through its
// symmetry, S[m][k] = S[k][m], so S is always read along its rows); the last one goes to global memory.
// SOLVE: h^2 / (lam_i + lam_j) after the second product, four products; else two (y = S x S).
// DIV: x / theta at the load (without it SOLVE is the plain L u = x, the preconditioner of poisson_div.hip).
// SHIFT (with SOLVE): dst_shift_scale after the second product instead, (L - sigma I) u = x.
constexpr int kFusedGroupTiles = 3;

static int dst_fused_np(int n) { return (n + 15) & ~15; }
static int dst_fused_waves(int n) {
  const int nt = dst_fused_np(n) / 16;
  return nt * ((nt + kFusedGroupTiles - 1) / kFusedGroupTiles);
}
static size_t dst_fused_lds(int n) {
  const int np = dst_fused_np(n);
  return (size_t)2 * np * (np + 2) * sizeof(double);
}

template <bool SOLVE, bool DIV, bool SHIFT>
__global__ __launch_bounds__(768) void dst_fused_kernel(const double* __restrict__ x, const double* __restrict__ th,
                                                        double* __restrict__ y, const double* __restrict__ S,
                                                        const double* __restrict__ lam, double h2, double inv_h2,
                                                        double sigma, int n) {
  extern __shared__ double dst_lds[];
  const int np = (n + 15) & ~15, ld = np + 2;
  double* Sl = dst_lds;
  double* Xl = dst_lds + np * ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long long base = (long long)blockIdx.x * n * n;
  const double* xb = x + base;
  const double* tb = DIV ? th + base : nullptr;
  double* yb = y + base;

  for (int i = tid; i < np * np; i += blockDim.x) {
    const int r = i / np, c = i - r * np;
    double sv = 0.0, xv = 0.0;
    if (r < n && c < n) {
      sv = S[r * n + c];
      xv = xb[r * n + c];
      if (DIV) xv = xv / tb[r * n + c];
    }
    Sl[r * ld + c] = sv;
    Xl[r * ld + c] = xv;
  }
  __syncthreads();

  const int nt = np / 16, ngrp = (nt + kFusedGroupTiles - 1) / kFusedGroupTiles;
  const int per = (nt + ngrp - 1) / ngrp;          // column tiles per group (<= 3)
  const int strip = wave / ngrp, grp = wave - strip * ngrp;
  const int ct0 = grp * per, ctn = min(nt, ct0 + per) - ct0;
  const int row0 = 16 * strip;
  const int ksteps = (n + 3) / 4;                  // k beyond n is zero in both buffers
  constexpr int nprod = SOLVE ? 4 : 2;

#pragma unroll 1
  for (int p = 0; p < nprod; ++p) {
    d4 acc[kFusedGroupTiles];
#pragma unroll
    for (int j = 0; j < kFusedGroupTiles; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    const bool xs = (p & 1) == 0;                  // X S; else S X
    const double* Am = xs ? Xl : Sl;
    const double* Bk = xs ? Sl : Xl;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int k = 4 * ks + l4;
      const double a = xs ? Am[(row0 + l15) * ld + k] : Am[k * ld + row0 + l15];
#pragma unroll
      for (int j = 0; j < kFusedGroupTiles; ++j)
        if (j < ctn) acc[j] = mfma_f64(a, Bk[k * ld + 16 * (ct0 + j) + l15], acc[j]);
    }
    const bool last = p == nprod - 1;
    if (!last) __syncthreads();                    // every wave has read Xl
#pragma unroll
    for (int j = 0; j < kFusedGroupTiles; ++j)
      if (j < ctn) {
        const int col = 16 * (ct0 + j) + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + l4 + 4 * r;
          const bool in = row < n && col < n;
          double v = acc[j][r];
          if (SOLVE && !SHIFT && p == 1) v = in ? v * (h2 / (lam[row] + lam[col])) : 0.0;
          if (SOLVE && SHIFT && p == 1) v = in ? v * dst_shift_scale(lam[row], lam[col], inv_h2, sigma) : 0.0;
          if (last) {
            if (in) yb[row * n + col] = v;
          } else {
            Xl[row * ld + col] = v;
          }
        }
      }
    if (!last) __syncthreads();
  }
}

// scale: 0 none, 1 h2 / (lam + lam), 2 dst_shift_scale with inv_h2 and sigma, 3 the same from two vectors
static int gemm_launch(bool div, int scale, const double* A, long long sA, const double* Bm, long long sB, double* C,
                       long long sC, const double* th, const double* lam, double h2, int n, int B, hipStream_t stream,
                       double inv_h2 = 0.0, double sigma = 0.0) {
  const int t = ceil_div(n, kGT);
  const dim3 grid(t, t, std::min(B, 65535)), block(256);
  if (div)
    hipLaunchKernelGGL((dst_gemm_kernel<true, 0>), grid, block, 0, stream, A, sA, Bm, sB, C, sC, th, lam, h2, inv_h2,
                       sigma, n, B);
  else if (scale == 1)
    hipLaunchKernelGGL((dst_gemm_kernel<false, 1>), grid, block, 0, stream, A, sA, Bm, sB, C, sC, th, lam, h2, inv_h2,
                       sigma, n, B);
  else if (scale == 2)
    hipLaunchKernelGGL((dst_gemm_kernel<false, 2>), grid, block, 0, stream, A, sA, Bm, sB, C, sC, th, lam, h2, inv_h2,
                       sigma, n, B);
  else if (scale == 3)
    hipLaunchKernelGGL((dst_gemm_kernel<false, 3>), grid, block, 0, stream, A, sA, Bm, sB, C, sC, th, lam, h2, inv_h2,
                       sigma, n, B);
  else
    hipLaunchKernelGGL((dst_gemm_kernel<false, 0>), grid, block, 0, stream, A, sA, Bm, sB, C, sC, th, lam, h2, inv_h2,
                       sigma, n, B);
  return 0;
}

// u = L^-1 (f / theta) for B problems, theta == nullptr: no division (u = L^-1 f).  sigma > 0 (theta == nullptr
// only): u = (L - sigma I)^-1 f; sigma = 0 is the unshifted code, kernel for kernel.  Arguments already checked.
int dst_solve_launch(const char* name, const double* f, const double* theta, double* u, int B, int n, const void* plan,
                     void* ws, hipStream_t stream, double sigma) {
  const double* S = static_cast<const double*>(plan);
  const double* lam = S + (size_t)n * n;
  const double h = 1.0 / (double)(n - 1), h2 = h * h;
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  const bool shift = sigma != 0.0;
  if (n <= kDstLdsMaxN) {
    const dim3 grid(B), block(64 * dst_fused_waves(n));
    if (shift)
      hipLaunchKernelGGL((dst_fused_kernel<true, false, true>), grid, block, dst_fused_lds(n), stream, f, theta, u, S,
                         lam, h2, inv_h2, sigma, n);
    else if (theta)
      hipLaunchKernelGGL((dst_fused_kernel<true, true, false>), grid, block, dst_fused_lds(n), stream, f, theta, u, S,
                         lam, h2, 0.0, 0.0, n);
    else
      hipLaunchKernelGGL((dst_fused_kernel<true, false, false>), grid, block, dst_fused_lds(n), stream, f, theta, u, S,
                         lam, h2, 0.0, 0.0, n);
    SRPDE_LAUNCH_CHECK(name);
    return 0;
  }
  const long long nn = (long long)n * n;
  double* w = static_cast<double*>(ws);
  gemm_launch(theta != nullptr, 0, f, nn, S, 0, w, nn, theta, lam, h2, n, B, stream);   // w = (f / theta) S
  SRPDE_LAUNCH_CHECK(name);
  // u = (S w) o h^2 / (lam + lam), or o dst_shift_scale
  gemm_launch(false, shift ? 2 : 1, S, 0, w, nn, u, nn, nullptr, lam, h2, n, B, stream, inv_h2, sigma);
  SRPDE_LAUNCH_CHECK(name);
  gemm_launch(false, 0, u, nn, S, 0, w, nn, nullptr, lam, h2, n, B, stream);  // w = u S
  SRPDE_LAUNCH_CHECK(name);
  gemm_launch(false, 0, S, 0, w, nn, u, nn, nullptr, lam, h2, n, B, stream);  // u = S w
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

size_t dst_plan_bytes_for(int n) { return dst_plan_bytes(n); }

// u = (L_bc - sigma I)^-1 f for B problems, the sides in the plan.  Arguments already checked; u must not alias f.
int sep_solve_launch(const char* name, const double* f, double* u, int B, int n, const void* plan, void* ws,
                     hipStream_t stream, double sigma) {
  const long long nn = (long long)n * n;
  const double* Qx = static_cast<const double*>(plan);
  const double *QxT = Qx + nn, *Qy = QxT + nn, *QyT = Qy + nn, *lam = QyT + nn;   // lam_y [n] then lam_x [n]
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  double* w = static_cast<double*>(ws);
  gemm_launch(false, 0, f, nn, Qx, 0, w, nn, nullptr, lam, 0.0, n, B, stream);                    // w = f Qx
  SRPDE_LAUNCH_CHECK(name);
  gemm_launch(false, 3, QyT, 0, w, nn, u, nn, nullptr, lam, 0.0, n, B, stream, inv_h2, sigma);    // u = (Qy^T w) o scale
  SRPDE_LAUNCH_CHECK(name);
  gemm_launch(false, 0, u, nn, QxT, 0, w, nn, nullptr, lam, 0.0, n, B, stream);                   // w = u Qx^T
  SRPDE_LAUNCH_CHECK(name);
  gemm_launch(false, 0, Qy, 0, w, nn, u, nn, nullptr, lam, 0.0, n, B, stream);                    // u = Qy w
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

size_t sep_plan_bytes_for(int n, int bc) { return sep_plan_bytes(n, bc); }

}  // namespace srpde

using namespace srpde;

extern "C" {

size_t srpde_poisson_dst_plan_size(int n) { return (n <= 0 || n > kDstMaxN) ? 0 : dst_plan_bytes(n); }

int srpde_poisson_dst_lds_max_n(void) { return kDstLdsMaxN; }

size_t srpde_poisson_dst_workspace_size(int B, int n) {
  if (B <= 0 || n <= kDstLdsMaxN || n > kDstMaxN) return 0;
  return (size_t)B * n * n * sizeof(double);
}

int srpde_poisson_dst_plan(int n, void* plan, size_t plan_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(plan, "srpde_poisson_dst_plan: null pointer");
  if (n <= 0 || n > kDstMaxN) SRPDE_FAIL(kErrShape, "srpde_poisson_dst_plan: bad shape n=%d (1 .. %d)", n, kDstMaxN);
  if (reinterpret_cast<uintptr_t>(plan) & 7u) SRPDE_FAIL(kErrAlign, "srpde_poisson_dst_plan: plan not 8-byte aligned");
  if (plan_bytes < dst_plan_bytes(n))
    SRPDE_FAIL(kErrWorkspace, "srpde_poisson_dst_plan: plan buffer too small (%zu bytes, n=%d needs %zu)", plan_bytes,
               n, dst_plan_bytes(n));
  double* S = static_cast<double*>(plan);
  hipLaunchKernelGGL(dst_plan_kernel, dim3(elementwise_grid((long long)n * n)), dim3(256), 0, stream, n, S,
                     S + (size_t)n * n);
  SRPDE_LAUNCH_CHECK("srpde_poisson_dst_plan");
  return 0;
}

// the checks srpde_poisson_dst_batched and srpde_poisson_dst_apply share; a plan is tied to its n by its size
static int dst_check(const char* name, int B, int n, int nmin, const void* plan, size_t plan_bytes, const void* ws,
                     size_t ws_bytes) {
  if (B <= 0 || n < nmin || n > kDstMaxN)
    SRPDE_FAIL(kErrShape, "%s: bad shape B=%d n=%d (B >= 1, n %d .. %d)", name, B, n, nmin, kDstMaxN);
  if (reinterpret_cast<uintptr_t>(plan) & 7u) SRPDE_FAIL(kErrAlign, "%s: plan not 8-byte aligned", name);
  if (plan_bytes != dst_plan_bytes(n))
    SRPDE_FAIL(kErrWorkspace, "%s: a plan of %zu bytes is not a plan for n=%d (srpde_poisson_dst_plan_size: %zu)", name,
               plan_bytes, n, dst_plan_bytes(n));
  if (n > kDstLdsMaxN) {
    if (!ws) SRPDE_FAIL(kErrArg, "%s: null workspace (n=%d > %d needs one)", name, n, kDstLdsMaxN);
    if (!aligned16(ws)) SRPDE_FAIL(kErrAlign, "%s: workspace not 16-byte aligned", name);
    if (ws_bytes < srpde_poisson_dst_workspace_size(B, n))
      SRPDE_FAIL(kErrWorkspace, "%s: workspace too small (%zu bytes, needs %zu)", name, ws_bytes,
                 srpde_poisson_dst_workspace_size(B, n));
  }
  return 0;
}

int srpde_poisson_dst_batched(const double* f, const double* theta, double* u, int B, int n, const void* plan,
                              size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  const char* name = "srpde_poisson_dst_batched";
  SRPDE_CHECK_ARG(f && theta && u && plan, "srpde_poisson_dst_batched: null pointer");
  if (int rc = dst_check(name, B, n, 2, plan, plan_bytes, ws, ws_bytes)) return rc;
  return dst_solve_launch(name, f, theta, u, B, n, plan, ws, stream);
}

int srpde_poisson_dst_shift_batched(const double* f, double* u, int B, int n, double sigma_p, const void* plan,
                                    size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  const char* name = "srpde_poisson_dst_shift_batched";
  SRPDE_CHECK_ARG(f && u && plan, "srpde_poisson_dst_shift_batched: null pointer");
  if (!(sigma_p >= 0.0) || !std::isfinite(sigma_p))
    SRPDE_FAIL(kErrArg, "srpde_poisson_dst_shift_batched: sigma_p=%g must be >= 0 and finite", sigma_p);
  if ((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(u)) & 7u)
    SRPDE_FAIL(kErrAlign, "srpde_poisson_dst_shift_batched: a pointer is not 8-byte aligned");
  if (int rc = dst_check(name, B, n, 2, plan, plan_bytes, ws, ws_bytes)) return rc;
  return dst_solve_launch(name, f, nullptr, u, B, n, plan, ws, stream, sigma_p);
}

size_t srpde_poisson_sep_plan_size(int n, int bc) {
  return (n < 2 || n > kDstMaxN || bc < 0 || bc > 15) ? 0 : sep_plan_bytes(n, bc);
}

size_t srpde_poisson_sep_workspace_size(int B, int n) {
  if (B <= 0 || n < 2 || n > kDstMaxN) return 0;
  return (size_t)B * n * n * sizeof(double);
}

int srpde_poisson_sep_plan(int n, int bc, void* plan, size_t plan_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(plan, "srpde_poisson_sep_plan: null pointer");
  if (n < 2 || n > kDstMaxN) SRPDE_FAIL(kErrShape, "srpde_poisson_sep_plan: bad shape n=%d (2 .. %d)", n, kDstMaxN);
  if (bc < 0 || bc > 15) SRPDE_FAIL(kErrArg, "srpde_poisson_sep_plan: bc=%d is not a side mask (0 .. 15)", bc);
  if (reinterpret_cast<uintptr_t>(plan) & 7u) SRPDE_FAIL(kErrAlign, "srpde_poisson_sep_plan: plan not 8-byte aligned");
  if (plan_bytes < sep_plan_bytes(n, bc))
    SRPDE_FAIL(kErrWorkspace, "srpde_poisson_sep_plan: plan buffer too small (%zu bytes, n=%d bc=%d needs %zu)",
               plan_bytes, n, bc, sep_plan_bytes(n, bc));
  // plan: Qx, Qx^T, Qy, Qy^T [n][n] each, lam_y [n], lam_x [n], then the mask as a double
  const size_t nn = (size_t)n * n;
  double* p = static_cast<double*>(plan);
  double *lam_y = p + 4 * nn, *lam_x = lam_y + n;
  const dim3 grid(elementwise_grid((long long)nn)), block(256);
  hipLaunchKernelGGL(sep_axis_kernel, grid, block, 0, stream, n, (bc >> 2) & 1, (bc >> 3) & 1, p, p + nn, lam_x,
                     lam_x + n, bc);
  hipLaunchKernelGGL(sep_axis_kernel, grid, block, 0, stream, n, bc & 1, (bc >> 1) & 1, p + 2 * nn, p + 3 * nn, lam_y,
                     static_cast<double*>(nullptr), bc);
  SRPDE_LAUNCH_CHECK("srpde_poisson_sep_plan");
  return 0;
}

int srpde_poisson_sep_shift_batched(const double* f, double* u, int B, int n, int bc, double sigma_p, const void* plan,
                                    size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  const char* name = "srpde_poisson_sep_shift_batched";
  SRPDE_CHECK_ARG(f && u && plan && ws, "srpde_poisson_sep_shift_batched: null pointer");
  if (B <= 0 || n < 2 || n > kDstMaxN)
    SRPDE_FAIL(kErrShape, "%s: bad shape B=%d n=%d (B >= 1, n 2 .. %d)", name, B, n, kDstMaxN);
  if (bc < 0 || bc > 15) SRPDE_FAIL(kErrArg, "%s: bc=%d is not a side mask (0 .. 15)", name, bc);
  if (!(sigma_p >= 0.0) || !std::isfinite(sigma_p))
    SRPDE_FAIL(kErrArg, "%s: sigma_p=%g must be >= 0 and finite", name, sigma_p);
  if (bc == 15 && sigma_p == 0.0)
    SRPDE_FAIL(kErrArg, "%s: four zero-flux sides (bc=15) with sigma_p=0 is singular (the constants)", name);
  if ((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(plan)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (u == f) SRPDE_FAIL(kErrArg, "%s: u aliases f (four launches: f is read after u is first written)", name);
  if (plan_bytes != sep_plan_bytes(n, bc))
    SRPDE_FAIL(kErrWorkspace, "%s: a plan of %zu bytes is not a plan for n=%d and bc=%d (srpde_poisson_sep_plan_size: %zu)",
               name, plan_bytes, n, bc, sep_plan_bytes(n, bc));
  if (!aligned16(ws)) SRPDE_FAIL(kErrAlign, "%s: workspace not 16-byte aligned", name);
  if (ws_bytes < srpde_poisson_sep_workspace_size(B, n))
    SRPDE_FAIL(kErrWorkspace, "%s: workspace too small (%zu bytes, needs %zu)", name, ws_bytes,
               srpde_poisson_sep_workspace_size(B, n));
  return sep_solve_launch(name, f, u, B, n, plan, ws, stream, sigma_p);
}

int srpde_poisson_dst_apply(const double* x, double* y, int B, int n, const void* plan, size_t plan_bytes, void* ws,
                            size_t ws_bytes, hipStream_t stream) {
  const char* name = "srpde_poisson_dst_apply";
  SRPDE_CHECK_ARG(x && y && plan, "srpde_poisson_dst_apply: null pointer");
  if (int rc = dst_check(name, B, n, 1, plan, plan_bytes, ws, ws_bytes)) return rc;
  const double* S = static_cast<const double*>(plan);
  const double* lam = S + (size_t)n * n;
  if (n <= kDstLdsMaxN) {
    hipLaunchKernelGGL((dst_fused_kernel<false, false, false>), dim3(B), dim3(64 * dst_fused_waves(n)),
                       dst_fused_lds(n), stream, x, nullptr, y, S, lam, 0.0, 0.0, 0.0, n);
    SRPDE_LAUNCH_CHECK(name);
    return 0;
  }
  const long long nn = (long long)n * n;
  double* w = static_cast<double*>(ws);
  gemm_launch(false, 0, x, nn, S, 0, w, nn, nullptr, lam, 0.0, n, B, stream);   // w = x S
  SRPDE_LAUNCH_CHECK(name);
  gemm_launch(false, 0, S, 0, w, nn, y, nn, nullptr, lam, 0.0, n, B, stream);   // y = S w
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

}  // extern "C"
