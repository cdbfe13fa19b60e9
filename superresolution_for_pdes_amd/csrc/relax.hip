// Weighted-Jacobi sweeps of  theta * L u = f  on an n x n grid, fp64, gfx950: the post-smoother of the cascade.
//
// Divided by theta the system is A u = h^2 f / theta with A the 5-point stencil (sum of the four neighbours minus
// 4x the centre, a zero ghost ring outside the grid).  One sweep, every operation rounded once, contraction off:
//
//     g  = f / (theta * inv_h2)                                   (once per node)
//     s  = (u[y-1][x] + u[y+1][x]) + (u[y][x-1] + u[y][x+1])      (a neighbour outside the grid is 0)
//     r  = (s - 4.0 * u) - g
//     u' = u + c * r                                              (c = 0.25 * omega, formed on the host)
//
// Jacobi: every u' comes from the previous sweep's u.  The error operator is I + (omega / 4) A, symmetric with
// eigenvalues 1 - omega (sin^2(a / 2) + sin^2(b / 2)): for 0 < omega <= 1 nothing grows.
//   interior_only = 0: all n^2 nodes move (the whole-domain operator of srpde_poisson_* / srpde_pde_residual_metrics);
//   interior_only = 1: the nodes with y or x in {0, n - 1} keep their input value (a crop whose ring is not zero).
//
// Temporal blocking: a workgroup owns a T x T output tile and stages the (T + 2K)^2 patch around it in LDS (positions
// outside the grid are 0), runs up to K sweeps ping-ponging two LDS planes and writes its centre.  The K-wide halo is
// the dependency cone of the centre, so no workgroup needs another one's result; sweep s of ks only computes the
// positions that the centre still depends on (those at least K - ks + s from the patch edge).  Positions outside the
// grid, and the ring under interior_only, are carried unchanged through every sweep ("fixed"), which is what makes
// the cone argument hold at the grid's edges.
//
// P = T + 2K = 64: a thread owns one patch column (its lane) and R = 8 consecutive rows (its wave, 8 waves).  Its
// eight u and g values live in registers for the whole launch, so a sweep reads from LDS only the left and right
// neighbours and the two rows above and below the wave's strip, and writes its new values for the neighbours.
// LDS: 2 planes x 64 x 64 x 8 B = 64 KiB, two workgroups (16 waves) per CU.  A row of 64 doubles covers the 64
// 4-byte banks twice over in one 32-lane group each: no bank conflicts.
//
// Every u' is a pure function of five values and g in a fixed order, so the result does not depend on T, K or how
// the sweeps are split over launches: it is bit-equal to one plain pass per sweep.
#include <cmath>

#include "common.h"
#include "relax_tile.h"

namespace srpde {
namespace {

// grid (tiles, tiles, E); ks <= K sweeps from u_in to u_out (ks = 0: a copy)
__global__ __launch_bounds__(kRelaxThreads) void pde_relax_kernel(const double* __restrict__ u_in,
                                                                  const double* __restrict__ f,
                                                                  const double* __restrict__ theta,
                                                                  double* __restrict__ u_out, int n, double inv_h2,
                                                                  double c, int ks, int interior_only) {
#pragma clang fp contract(off)
  constexpr int P = kRelaxP, K = kRelaxK, T = kRelaxT, R = kRelaxR;
  __shared__ double plane[2][P * P];
  const int x = threadIdx.x & 63, y0 = (threadIdx.x >> 6) * R;
  const int gx = (int)blockIdx.x * T - K + x, gy0 = (int)blockIdx.y * T - K + y0;
  const long long base = (long long)blockIdx.z * n * n;
  const bool col_in = gx >= 0 && gx < n;
  const bool col_fixed = !col_in || (interior_only && (gx == 0 || gx == n - 1));

  double uc[R], g[R];
  unsigned fixed = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gy = gy0 + r;
    const bool row_in = gy >= 0 && gy < n;
    double uv = 0.0, gv = 0.0;
    if (col_in && row_in) {
      const long long k = base + (long long)gy * n + gx;
      uv = u_in[k];
      gv = f[k] / (theta[k] * inv_h2);
    }
    uc[r] = uv;
    g[r] = gv;
    if (col_fixed || !row_in || (interior_only && (gy == 0 || gy == n - 1))) fixed |= 1u << r;
    plane[0][(y0 + r) * P + x] = uv;
  }
  __syncthreads();

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
        const double sum = (prev + dn) + (in[y * P + x - 1] + in[y * P + x + 1]);
        const double res = (sum - 4.0 * cur) - g[r];
        const double nv = (fixed >> r) & 1u ? cur : cur + c * res;
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

int srpde_pde_relax_sweeps_per_launch(void) { return kRelaxK; }

size_t srpde_pde_relax_workspace_size(int E, int n, int sweeps) {
  if (E <= 0 || n < 1 || sweeps <= kRelaxK) return 0;
  return (size_t)E * n * n * sizeof(double);
}

int srpde_pde_relax(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                    double inv_h2, int sweeps, double omega, int interior_only, void* workspace, size_t ws_bytes,
                    hipStream_t stream) {
  SRPDE_CHECK_ARG(u_in && f && theta && u_out, "srpde_pde_relax: null pointer");
  if (E <= 0 || E > 65535 || n < 1 || n > kRelaxMaxN || (interior_only && n < 3))
    SRPDE_FAIL(kErrShape, "srpde_pde_relax: bad shape E=%d n=%d (1 <= E <= 65535, 1 <= n <= %d, interior_only needs n >= 3)",
               E, n, kRelaxMaxN);
  if (sweeps < 0) SRPDE_FAIL(kErrArg, "srpde_pde_relax: sweeps=%d is negative", sweeps);
  if (!(omega > 0.0 && omega <= 1.0)) SRPDE_FAIL(kErrArg, "srpde_pde_relax: omega=%g outside (0, 1]", omega);
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "srpde_pde_relax: inv_h2=%g must be positive and finite", inv_h2);
  const size_t bytes = (size_t)E * n * n * sizeof(double);
  const size_t need = srpde_pde_relax_workspace_size(E, n, sweeps);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(u_in) | reinterpret_cast<uintptr_t>(f) |
                         reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(u_out) |
                         (need ? reinterpret_cast<uintptr_t>(workspace) : 0);
  if (bits & 7u) SRPDE_FAIL(kErrAlign, "srpde_pde_relax: a pointer is not 8-byte aligned");
  if (relax_overlap(u_out, u_in, bytes) || relax_overlap(u_out, f, bytes) || relax_overlap(u_out, theta, bytes))
    SRPDE_FAIL(kErrArg, "srpde_pde_relax: u_out overlaps an input (a sweep reads its neighbours' old values)");
  if (need) {
    if (workspace == nullptr || ws_bytes < need) SRPDE_FAIL(kErrWorkspace, "srpde_pde_relax: workspace too small");
    if (relax_overlap(workspace, u_out, bytes) || relax_overlap(workspace, u_in, bytes) ||
        relax_overlap(workspace, f, bytes) || relax_overlap(workspace, theta, bytes))
      SRPDE_FAIL(kErrArg, "srpde_pde_relax: the workspace overlaps a field");
  }
  const double c = 0.25 * omega;
  const int tiles = ceil_div(n, kRelaxT);
  const int launches = std::max(1, ceil_div(sweeps, kRelaxK));
  double* ws = static_cast<double*>(workspace);
  const double* src = u_in;
  for (int j = 0; j < launches; ++j) {
    // the last launch writes u_out, the one before it the workspace, and so on backwards
    double* dst = ((launches - 1 - j) & 1) ? ws : u_out;
    const int ks = std::min(kRelaxK, sweeps - j * kRelaxK);
    hipLaunchKernelGGL(pde_relax_kernel, dim3(tiles, tiles, E), dim3(kRelaxThreads), 0, stream, src, f, theta, dst, n,
                       inv_h2, c, ks, interior_only);
    SRPDE_LAUNCH_CHECK("srpde_pde_relax");
    src = dst;
  }
  return 0;
}

}  // extern "C"
