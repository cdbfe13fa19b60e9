// Weighted-Jacobi sweeps of the divergence-form equation  div(theta grad u) = f  on an n x n grid, fp64, gfx950: the
// post-smoother of a cascade whose samples solve the conservative problem (poisson_div.hip).
//
// The operator is that of srpde_div_apply.  Face coefficient between node a and its neighbour b: 0.5 * (ta + tb)
// (face_mean 0) or (2.0 * (ta * tb)) / (ta + tb) (face_mean 1); towards the ghost ring c = ta and u_b = 0.  One sweep,
// every operation rounded once, contraction off for the whole file:
//
//     once per node:   g = f / inv_h2
//                      w = omega / ((cE + cW) + (cS + cN))
//     per sweep:       a  = (cE*(uE - u) + cW*(uW - u)) + (cS*(uS - u) + cN*(uN - u))
//                      u' = u + w * (a - g)
//
// (E is x + 1, S is y + 1.)  Jacobi: every u' comes from the previous sweep's u.  The error operator is
// I - omega diag(-D_theta)^-1 (-D_theta); -D_theta is a symmetric, weakly diagonally dominant M-matrix, so the Jacobi
// spectrum lies in [0, 2] and for 0 < omega <= 1 nothing grows.  interior_only as in relax.hip: the ring keeps its
// input values (a crop whose ring is not zero).
//
// Temporal blocking is that of pde_relax_kernel (relax_tile.h): a 64^2 patch = 48^2 tile + an 8-wide halo, one lane
// per patch column, 8 rows per thread, u ping-ponged between two LDS planes, up to 8 sweeps per launch.  What is new
// is the sweep-invariant data: g, w and the four face coefficients.  They are formed once per launch while staging --
// theta goes through the LDS plane that sweep 1 overwrites -- and then live in registers, so the harmonic mean's
// divisions are paid once per launch and no coefficient touches global memory or LDS between sweeps:
//     u[8], g[8], w[8]                 24 doubles
//     cE[8]                             8   (the face towards x + 1)
//     cW[8]                             8   = cE of lane x - 1, fetched once per launch with a wave shuffle (a wave is
//                                           one patch row); the means are commutative, so the bits are the same
//     cV[9]                             9   cV[r] is the face between rows r - 1 and r: cN of row r and cS of row r - 1
// 49 doubles = 98 VGPRs.  A face with exactly one end inside the grid carries theta of that end (the ghost-face rule
// of the in-grid node; the outside node is fixed at 0 and never reads it), a face with no end inside carries 1.
// Positions outside the grid and, under interior_only, the ring are carried unchanged through every sweep.
//
// Every u' is a pure function of its five u values and the node's constants in a fixed order: the result is bit-equal
// to one plain pass per sweep, whatever the tiling or the launch split.
#include <cmath>

#include "common.h"
#include "relax_tile.h"

#pragma clang fp contract(off)

namespace srpde {
namespace {

// the coefficient of the face between positions a and b (theta 1 is staged outside the grid, so the mean is finite)
template <bool HARM>
__device__ __forceinline__ double relax_face(double ta, double tb, bool in_a, bool in_b) {
  const double m = HARM ? (2.0 * (ta * tb)) / (ta + tb) : 0.5 * (ta + tb);
  return in_a && in_b ? m : (in_a ? ta : tb);
}

// grid (tiles, tiles, E); ks <= K sweeps from u_in to u_out (ks = 0: a copy)
template <bool HARM>
__global__ __launch_bounds__(kRelaxThreads) void div_relax_kernel(const double* __restrict__ u_in,
                                                                  const double* __restrict__ f,
                                                                  const double* __restrict__ theta,
                                                                  double* __restrict__ u_out, int n, double inv_h2,
                                                                  double omega, int ks, int interior_only) {
  constexpr int P = kRelaxP, K = kRelaxK, T = kRelaxT, R = kRelaxR;
  __shared__ double plane[2][P * P];
  const int x = threadIdx.x & 63, y0 = (threadIdx.x >> 6) * R;
  const int gx = (int)blockIdx.x * T - K + x, gy0 = (int)blockIdx.y * T - K + y0;
  const long long base = (long long)blockIdx.z * n * n;
  const bool col_in = gx >= 0 && gx < n;
  const bool col_in_e = gx + 1 >= 0 && gx + 1 < n;
  const bool col_fixed = !col_in || (interior_only && (gx == 0 || gx == n - 1));

  double uc[R], g[R], w[R], cE[R], cW[R], cV[R + 1];
  unsigned fixed = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gy = gy0 + r;
    const bool row_in = gy >= 0 && gy < n;
    double uv = 0.0, gv = 0.0, tv = 1.0;
    if (col_in && row_in) {
      const long long k = base + (long long)gy * n + gx;
      uv = u_in[k];
      gv = f[k] / inv_h2;
      tv = theta[k];
    }
    uc[r] = uv;
    g[r] = gv;
    if (col_fixed || !row_in || (interior_only && (gy == 0 || gy == n - 1))) fixed |= 1u << r;
    plane[0][(y0 + r) * P + x] = uv;
    plane[1][(y0 + r) * P + x] = tv;
  }
  __syncthreads();

  {
    const double* th = plane[1];
    // the face above the strip's first row; a strip at the patch's top edge has none (that row is never live)
    double t_prev = y0 > 0 ? th[(y0 - 1) * P + x] : 1.0;
    bool in_prev = col_in && y0 > 0 && gy0 - 1 >= 0 && gy0 - 1 < n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int y = y0 + r, gy = gy0 + r;
      const bool row_in = gy >= 0 && gy < n;
      const bool in_c = col_in && row_in;
      const double tc = th[y * P + x];
      const double te = x + 1 < P ? th[y * P + x + 1] : 1.0;
      cV[r] = relax_face<HARM>(tc, t_prev, in_c, in_prev);
      cE[r] = relax_face<HARM>(tc, te, in_c, col_in_e && row_in && x + 1 < P);
      t_prev = tc;
      in_prev = in_c;
    }
    const bool below_in = y0 + R < P && col_in && gy0 + R >= 0 && gy0 + R < n;
    const double t_below = y0 + R < P ? th[(y0 + R) * P + x] : 1.0;
    cV[R] = relax_face<HARM>(t_prev, t_below, in_prev, below_in);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cW[r] = __shfl_up(cE[r], 1, 64);                 // lane 0 keeps its own: patch column 0 is never live
      w[r] = omega / ((cE[r] + cW[r]) + (cV[r + 1] + cV[r]));
    }
  }
  __syncthreads();                                     // sweep 1 writes the plane theta was staged in

  for (int s = 1; s <= ks; ++s) {
    const double* in = plane[(s - 1) & 1];
    double* out = plane[s & 1];
    const int lo = K - ks + s, hi = P - 1 - lo;        // 1 <= lo: x - 1 and x + 1 stay inside the row
    const bool x_live = x >= lo && x <= hi;
    double prev = y0 > 0 ? in[(y0 - 1) * P + x] : 0.0;
    const double below = y0 + R < P ? in[(y0 + R) * P + x] : 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int y = y0 + r;
      const double cur = uc[r];
      const double dn = r + 1 < R ? uc[r + 1] : below;
      if (x_live && y >= lo && y <= hi) {
        const double uE = in[y * P + x + 1], uW = in[y * P + x - 1];
        const double a = (cE[r] * (uE - cur) + cW[r] * (uW - cur)) + (cV[r + 1] * (dn - cur) + cV[r] * (prev - cur));
        const double nv = (fixed >> r) & 1u ? cur : cur + w[r] * (a - g[r]);
        uc[r] = nv;
        out[y * P + x] = nv;
      }
      prev = cur;
    }
    __syncthreads();
  }

  if (x >= K && x < K + T && gx < n) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int y = y0 + r, gy = gy0 + r;
      if (y >= K && y < K + T && gy < n) u_out[base + (long long)gy * n + gx] = uc[r];
    }
  }
}

}  // namespace
}  // namespace srpde

using namespace srpde;

extern "C" {

size_t srpde_div_relax_workspace_size(int E, int n, int sweeps) {
  if (E <= 0 || n < 1 || sweeps <= kRelaxK) return 0;
  return (size_t)E * n * n * sizeof(double);
}

int srpde_div_relax(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                    int face_mean, double inv_h2, int sweeps, double omega, int interior_only, void* workspace,
                    size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_in && f && theta && u_out, "srpde_div_relax: null pointer");
  if (E <= 0 || E > 65535 || n < 1 || n > kRelaxMaxN || (interior_only && n < 3))
    SRPDE_FAIL(kErrShape, "srpde_div_relax: bad shape E=%d n=%d (1 <= E <= 65535, 1 <= n <= %d, interior_only needs n >= 3)",
               E, n, kRelaxMaxN);
  if (face_mean != 0 && face_mean != 1)
    SRPDE_FAIL(kErrArg, "srpde_div_relax: face_mean=%d (0 arithmetic, 1 harmonic)", face_mean);
  if (sweeps < 0) SRPDE_FAIL(kErrArg, "srpde_div_relax: sweeps=%d is negative", sweeps);
  if (!(omega > 0.0 && omega <= 1.0)) SRPDE_FAIL(kErrArg, "srpde_div_relax: omega=%g outside (0, 1]", omega);
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "srpde_div_relax: inv_h2=%g must be positive and finite", inv_h2);
  const size_t bytes = (size_t)E * n * n * sizeof(double);
  const size_t need = srpde_div_relax_workspace_size(E, n, sweeps);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(u_in) | reinterpret_cast<uintptr_t>(f) |
                         reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(u_out) |
                         (need ? reinterpret_cast<uintptr_t>(workspace) : 0);
  if (bits & 7u) SRPDE_FAIL(kErrAlign, "srpde_div_relax: a pointer is not 8-byte aligned");
  if (relax_overlap(u_out, u_in, bytes) || relax_overlap(u_out, f, bytes) || relax_overlap(u_out, theta, bytes))
    SRPDE_FAIL(kErrArg, "srpde_div_relax: u_out overlaps an input (a sweep reads its neighbours' old values)");
  if (need) {
    if (workspace == nullptr || ws_bytes < need) SRPDE_FAIL(kErrWorkspace, "srpde_div_relax: workspace too small");
    if (relax_overlap(workspace, u_out, bytes) || relax_overlap(workspace, u_in, bytes) ||
        relax_overlap(workspace, f, bytes) || relax_overlap(workspace, theta, bytes))
      SRPDE_FAIL(kErrArg, "srpde_div_relax: the workspace overlaps a field");
  }
  const int tiles = ceil_div(n, kRelaxT);
  const int launches = std::max(1, ceil_div(sweeps, kRelaxK));
  double* ws = static_cast<double*>(workspace);
  const double* src = u_in;
  for (int j = 0; j < launches; ++j) {
    // the last launch writes u_out, the one before it the workspace, and so on backwards
    double* dst = ((launches - 1 - j) & 1) ? ws : u_out;
    const int ks = std::min(kRelaxK, sweeps - j * kRelaxK);
    if (face_mean)
      hipLaunchKernelGGL(div_relax_kernel<true>, dim3(tiles, tiles, E), dim3(kRelaxThreads), 0, stream, src, f, theta,
                         dst, n, inv_h2, omega, ks, interior_only);
    else
      hipLaunchKernelGGL(div_relax_kernel<false>, dim3(tiles, tiles, E), dim3(kRelaxThreads), 0, stream, src, f, theta,
                         dst, n, inv_h2, omega, ks, interior_only);
    SRPDE_LAUNCH_CHECK("srpde_div_relax");
    src = dst;
  }
  return 0;
}

}  // extern "C"
