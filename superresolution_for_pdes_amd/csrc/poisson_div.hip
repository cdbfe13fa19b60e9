// Divergence-form Poisson operator  D_theta u = div(theta grad u) = f  and its sine-preconditioned CG, fp64, gfx950.
//
// Grid: all n^2 nodes unknown, a zero ghost ring one h outside, h = 1 / (n - 1).  For node a with nodal theta_a and
// neighbour b the face coefficient is
//     arithmetic (face_mean 0):  c = 0.5 * (ta + tb)
//     harmonic   (face_mean 1):  c = (2.0 * (ta * tb)) / (ta + tb)
//     b outside the grid:        c = ta, u_b = 0
// and, every operation rounded once in this order (contraction is off for the whole file),
//     y = ((cE*(uE - u) + cW*(uW - u)) + (cS*(uS - u) + cN*(uN - u))) * inv_h2
// c is bit-symmetric in (a, b), so D_theta is exactly symmetric; it is negative definite, and for a constant theta it
// is theta * L (L the 5-point Laplacian of poisson.hip / poisson_dst.hip).
//
// Both D_theta and L are sums over the same faces with coefficients c and 1, so theta_min (-L) <= -D_theta <=
// theta_max (-L): with M = L, solved exactly by the sine transform, cond(M^-1 D_theta) <= theta_max / theta_min for
// every n, and CG needs a number of iterations that does not grow with n.
//
//     x = 0;  r = f;  z = M^-1 r;  p = z
//     k = 1, 2, ...:  alpha = (r.z) / (p.D p);  x += alpha p;  r -= alpha D p
//                     the problem stops when |r| <= rtol |f|
//                     z = M^-1 r;  beta = (r.z)_new / (r.z)_old;  p = z + beta p
//
// Launches of iteration k (grid: 64 x 32-node tiles x B problems, 256 threads, a thread owns one column of 8 rows):
//   (a) div_apply_kernel<PCG>  beta from the r.z partials of the two previous (d); p = z + beta p for the tile and its
//                              one-node halo, staged in LDS with theta (k = 1: p = z); stores p (into the other of
//                              two p buffers: a neighbour block still reads the old one for its halo), q = D p and
//                              the block's partial of p.q
//   (b) div_update_kernel      alpha from the partials; x += alpha p, r -= alpha q; the block's partial of r.r
//   (c) the sine-transform solve z = L^-1 r (poisson_dst.h: no division by a coefficient)
//   (d) div_rz_kernel          the block's partial of r.z; block 0 of each problem sums the r.r partials and sets the
//                              problem's iteration count, residual and done flag
// Every block that needs a scalar re-sums the problem's partials itself, in one fixed order, so all blocks of a problem
// get the same bits: no atomics, no grid barrier, no cooperative launch, no host sync.  A problem's arithmetic sees
// nothing of the other problems, so its result does not depend on B or on its place in the batch.
//
// Freeze rule.  done[b] is written only by (d) and read only by the (a) and (b) after it.  Once set, (a) and (b)
// return at once for that problem: x, r, p, iters and resid stay as they are, no 0/0 is formed, and further
// iterations are harmless.  |f| = 0 sets done in init's (d): x = 0 exactly, iters = 0, resid = 0.
//
// Warm start (srpde_div_cg_init_from).  x = u0, r = f - D u0 in one fused pass (div_init_from_kernel), z = M^-1 r,
// then div_rz_from_kernel, the k = 0 pass that keeps |f| apart from |r0| and decides done at the real rtol.  The
// iterations above run unchanged on that state; the zero-start kernels are not touched.
//
// Shift (srpde_div_apply_shift, srpde_div_cg_*_shift, srpde_div_step_rhs).  A = D_theta - sigma I, sigma >= 0, is the
// operator of an implicit time step of u_t = D_theta u - f (sigma = 1 / dt) and of the screened problem.  It is as
// symmetric and negative definite as D_theta, and with M = L - sigma_p I, sigma_p = sigma / theta_g for any theta_g in
// [theta_min, theta_max], min(theta_min, theta_g) (-M) <= -A <= max(theta_max, theta_g) (-M): cond(M^-1 A) <=
// theta_max / theta_min for every n and every sigma.  The shift is a template argument of div_apply_kernel and
// div_init_from_kernel, y = D u - sigma * u as one product and one subtraction after the face sum's * inv_h2, and an
// argument of the sine-transform solve (poisson_dst.h); everything else of the iteration -- update, r.z, the freeze
// rule, the fixed-order sums, finish -- is the code above, untouched.  sigma = 0 launches the unshifted kernels.
//
// Boundary pattern (the *_bc entries).  bc is a 4-bit mask, bit 0 the row 0 side, bit 1 the row n - 1 side, bit 2 the
// column 0 side, bit 3 the column n - 1 side; a set bit is a zero-flux side: its ghost faces are missing (coefficient
// 0), a clear bit is the zero ghost ring above.  The operator stays a sum over faces with c in [theta_min, theta_max],
// and so does M = L_bc - sigma_p I, the constant-coefficient operator with the same sides, which poisson_dst.hip's
// separable solve inverts exactly: cond(M^-1 A) <= theta_max / theta_min for every n, sigma and pattern.  All four sides
// zero-flux with sigma = 0 is singular (the constants) and refused.  The kernels are the tile bodies below with BC set
// (face_sum_bc / face_grad_sum_bc in place of face_sum / face_grad_sum) and step (c) is the separable solve; update,
// r.z, the k = 0 pass, the freeze rule and finish are the code above, untouched.
//
// Boundary data (the *_bd entries).  bd [Bd][4][n] gives the sides values: the ghost value g beyond a Dirichlet side's
// edge node, the outward flux q through a zero-flux side's ghost face (div_stencil.h).  A_bd u = D_bc u - sigma u + b:
// the tile bodies with BD set stage g into the out-of-grid halo of u (bd_halo, reached only by entries outside the
// grid) and add ((qE + qW) + (qS + qN)) * inv_h at flux-side nodes after the face sum's * inv_h2.  The solve is
// (D_bc - sigma I) u = f - b: srpde_div_cg_init_from_bd forms r = f - A_bd u0 and the partials of (f - b)^2, the stop
// rule's reference, in one pass on either workspace (mask 0: the sine plan's), and the iteration above runs unchanged.
//
// Adjoint (srpde_div_theta_grad).  D_theta is symmetric, so the adjoint of the solve is the same solve, and the
// gradient in theta of <lam, D_theta u> is the local pair gradient G(u, lam; theta) of div_theta_grad_kernel.
#include <cmath>

#include "common.h"
#include "field_reduce.h"
#include "poisson_dst.h"

#pragma clang fp contract(off)
#include "div_stencil.h"                   // after the pragma: its functions take the mode of this file

namespace srpde {
namespace {

constexpr int kDivTX = 64;                 // tile width: one column per lane
constexpr int kDivTY = 32;                 // tile height
constexpr int kDivThreads = 256;
constexpr int kDivR = kDivTY / (kDivThreads / 64);   // rows per thread
constexpr int kDivLX = kDivTX + 2, kDivLY = kDivTY + 2;
constexpr int kDivMaxN = 16384;
constexpr int kDivMaxB = 65535;
static_assert(kDivR * (kDivThreads / 64) == kDivTY, "the waves' strips tile the tile");
static_assert(kDivThreads == kRedThreads, "block_sum and resum (field_reduce.h) reduce over 256 threads");

struct DivCG {
  double *x, *r, *z, *q, *p[2];            // [B][n][n]
  double *prr, *ppq, *prz[2];              // [B][nb] per-block partials
  double *ff, *resid;                      // [B]
  int *iters, *done;                       // [B]
  void* dst_ws;
  void* sep_ws;                            // the separable solve's field (carve with bc only)
  int n, nb;
  size_t bytes;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// bc: the layout of the *_bc entries -- the same offsets, so srpde_div_cg_finish and the done flags serve both, plus
// the separable solve's [B][n][n] field at the end where the sine solve's workspace is empty (n up to its LDS limit)
DivCG carve(void* ws, int B, int n, bool bc = false) {
  DivCG g;
  char* c = static_cast<char*>(ws);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* p = c + at;
    at += up16(bytes);
    return p;
  };
  const size_t field = (size_t)B * n * n * sizeof(double);
  g.n = n;
  g.nb = ceil_div(n, kDivTX) * ceil_div(n, kDivTY);
  const size_t part = (size_t)B * g.nb * sizeof(double);
  g.x = reinterpret_cast<double*>(take(field));
  g.r = reinterpret_cast<double*>(take(field));
  g.z = reinterpret_cast<double*>(take(field));
  g.q = reinterpret_cast<double*>(take(field));
  g.p[0] = reinterpret_cast<double*>(take(field));
  g.p[1] = reinterpret_cast<double*>(take(field));
  g.dst_ws = take(srpde_poisson_dst_workspace_size(B, n));
  g.prr = reinterpret_cast<double*>(take(part));
  g.ppq = reinterpret_cast<double*>(take(part));
  g.prz[0] = reinterpret_cast<double*>(take(part));
  g.prz[1] = reinterpret_cast<double*>(take(part));
  g.ff = reinterpret_cast<double*>(take((size_t)B * sizeof(double)));
  g.resid = reinterpret_cast<double*>(take((size_t)B * sizeof(double)));
  g.iters = reinterpret_cast<int*>(take((size_t)B * sizeof(int)));
  g.done = reinterpret_cast<int*>(take((size_t)B * sizeof(int)));
  g.sep_ws = g.dst_ws;
  if (bc && srpde_poisson_dst_workspace_size(B, n) == 0) g.sep_ws = take(field);
  g.bytes = at;
  return g;
}

// block_sum and resum (field_reduce.h) give the same bits in every thread.  red, their 4 doubles of LDS, is used for
// nothing else in these kernels, and each call's first barrier comes before its write, so back-to-back calls are safe.

__device__ __forceinline__ int block_id() { return (int)(blockIdx.y * gridDim.x + blockIdx.x); }

// the face sum / pair-gradient sum of node (gx, gy), whose halo tiles start at LDS offset c; BC: with the side mask bc
template <bool HARM, bool BC>
__device__ __forceinline__ double node_face_sum(const double* us, const double* ts, int c, int gx, int gy, int n,
                                                int bc) {
  if (BC)
    return face_sum_bc<HARM>(us + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n, !(bc & 4), !(bc & 8),
                             !(bc & 1), !(bc & 2));
  return face_sum<HARM>(us + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n);
}

template <bool HARM, bool BC>
__device__ __forceinline__ double node_face_grad_sum(const double* us, const double* ls, const double* ts, int c,
                                                     int gx, int gy, int n, int bc) {
  if (BC)
    return face_grad_sum_bc<HARM>(us + c, ls + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n, !(bc & 4),
                                  !(bc & 8), !(bc & 1), !(bc & 2));
  return face_grad_sum<HARM>(us + c, ls + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n);
}

// y = D_theta u for one tile.  PCG: u = p = z + beta p_old is formed here (header, launch (a)).
// SHIFT: y = D_theta u - sigma * u (the product, then the subtraction, after the face sum's * inv_h2).
// BC: with the side mask bc (the body of div_apply_kernel and div_apply_bc_kernel).
// BD (with BC, of div_apply_bd_kernel): bd is the problem's boundary data; the out-of-grid halo of u holds g beyond
// Dirichlet sides (bd_halo) and a node on a flux side gains bd_flux_sum * inv_h after the face sum's * inv_h2.
template <bool PCG, bool HARM, bool SHIFT, bool BC, bool BD = false>
__device__ __forceinline__ void div_apply_tile(const double* __restrict__ u, const double* __restrict__ theta,
                                               double* __restrict__ y, const DivCG& g, double inv_h2, double sigma,
                                               int n, int k, int bc, const double* __restrict__ bd = nullptr,
                                               double inv_h = 0.0) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z;
  const long long base = (long long)b * n * n;
  const int x0 = (int)blockIdx.x * kDivTX, y0 = (int)blockIdx.y * kDivTY;
  double beta = 0.0;
  const double* pold = nullptr;
  double* pnew = nullptr;
  if (PCG) {
    if (g.done[b]) return;                 // the same for the whole block
    pnew = g.p[k & 1];
    if (k > 1) {
      pold = g.p[(k - 1) & 1];
      const double rz_new = resum(g.prz[(k - 1) & 1] + (size_t)b * g.nb, g.nb, red);
      const double rz_old = resum(g.prz[k & 1] + (size_t)b * g.nb, g.nb, red);
      beta = rz_old != 0.0 ? rz_new / rz_old : 0.0;
    }
  }
  for (int i = tid; i < kDivLY * kDivLX; i += kDivThreads) {
    const int ly = i / kDivLX, lx = i - ly * kDivLX;
    const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    double uv = 0.0, tv = 1.0;
    if (gy >= 0 && gy < n && gx >= 0 && gx < n) {
      const long long at = base + (long long)gy * n + gx;
      uv = u[at];
      tv = theta[at];
      if (PCG && k > 1) uv = uv + beta * pold[at];
    } else if (BD) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ts[i] = tv;
  }
  __syncthreads();

  const int lx = (tid & 63) + 1, gx = x0 + (tid & 63);
  const int ly0 = (tid >> 6) * kDivR + 1;
  double acc = 0.0;
  if (gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int ly = ly0 + r, gy = y0 + ly - 1;
      if (gy < n) {
        const int c = ly * kDivLX + lx;
        const double uc = us[c];
        double yv = node_face_sum<HARM, BC>(us, ts, c, gx, gy, n, bc) * inv_h2;
        if (BD && bd_flux_node(gy, gx, n, bc)) yv = yv + bd_flux_sum(bd, gy, gx, n, bc) * inv_h;
        if (SHIFT) yv = yv - sigma * uc;
        const long long at = base + (long long)gy * n + gx;
        y[at] = yv;
        if (PCG) {
          pnew[at] = uc;
          acc = acc + uc * yv;
        }
      }
    }
  }
  if (PCG) {
    const double s = block_sum(acc, red);
    if (tid == 0) g.ppq[(size_t)b * g.nb + block_id()] = s;
  }
}

template <bool PCG, bool HARM, bool SHIFT>
__global__ __launch_bounds__(kDivThreads) void div_apply_kernel(const double* __restrict__ u,
                                                                const double* __restrict__ theta,
                                                                double* __restrict__ y, DivCG g, double inv_h2,
                                                                double sigma, int n, int k) {
  div_apply_tile<PCG, HARM, SHIFT, false>(u, theta, y, g, inv_h2, sigma, n, k, 0);
}

template <bool PCG, bool HARM, bool SHIFT>
__global__ __launch_bounds__(kDivThreads) void div_apply_bc_kernel(const double* __restrict__ u,
                                                                   const double* __restrict__ theta,
                                                                   double* __restrict__ y, DivCG g, double inv_h2,
                                                                   double sigma, int n, int k, int bc) {
  div_apply_tile<PCG, HARM, SHIFT, true>(u, theta, y, g, inv_h2, sigma, n, k, bc);
}

// y = A_bd u = D_theta u - sigma * u + b(bd, theta) (srpde_div_apply_bd); bd_stride: 4 n, or 0 for one [4][n] shared
template <bool HARM, bool SHIFT>
__global__ __launch_bounds__(kDivThreads) void div_apply_bd_kernel(const double* __restrict__ u,
                                                                   const double* __restrict__ theta,
                                                                   double* __restrict__ y, double inv_h2, double sigma,
                                                                   int n, int bc, const double* __restrict__ bd,
                                                                   long long bd_stride, double inv_h) {
  const DivCG none = {};
  div_apply_tile<false, HARM, SHIFT, true, true>(u, theta, y, none, inv_h2, sigma, n, 0, bc,
                                                 bd + (long long)blockIdx.z * bd_stride, inv_h);
}

// launch (b): x += alpha p, r -= alpha q, partial of r.r
__global__ __launch_bounds__(kDivThreads) void div_update_kernel(DivCG g, int k) {
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  if (g.done[b]) return;
  const double pq = resum(g.ppq + (size_t)b * g.nb, g.nb, red);
  const double rz = resum(g.prz[(k - 1) & 1] + (size_t)b * g.nb, g.nb, red);
  const double alpha = pq != 0.0 ? rz / pq : 0.0;
  const double* __restrict__ p = g.p[k & 1];
  const long long base = (long long)b * n * n;
  const int gx = (int)blockIdx.x * kDivTX + (tid & 63);
  const int gy0 = (int)blockIdx.y * kDivTY + (tid >> 6) * kDivR;
  double acc = 0.0;
  if (gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int gy = gy0 + r;
      if (gy < n) {
        const long long at = base + (long long)gy * n + gx;
        g.x[at] = g.x[at] + alpha * p[at];
        const double rv = g.r[at] - alpha * g.q[at];
        g.r[at] = rv;
        acc = acc + rv * rv;
      }
    }
  }
  const double s = block_sum(acc, red);
  if (tid == 0) g.prr[(size_t)b * g.nb + block_id()] = s;
}

// launch (d): partial of r.z; block 0 of a problem settles iteration k (k = 0: the state after init)
__global__ __launch_bounds__(kDivThreads) void div_rz_kernel(DivCG g, int k, double rtol) {
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  const long long base = (long long)b * n * n;
  const int gx = (int)blockIdx.x * kDivTX + (tid & 63);
  const int gy0 = (int)blockIdx.y * kDivTY + (tid >> 6) * kDivR;
  double acc = 0.0;
  if (gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int gy = gy0 + r;
      if (gy < n) {
        const long long at = base + (long long)gy * n + gx;
        acc = acc + g.r[at] * g.z[at];
      }
    }
  }
  const double s = block_sum(acc, red);
  if (tid == 0) g.prz[k & 1][(size_t)b * g.nb + block_id()] = s;
  if (block_id() != 0) return;
  const bool was_done = k > 0 && g.done[b] != 0;     // read by every thread before resum's barriers, written after them
  if (was_done) return;
  const double rr = resum(g.prr + (size_t)b * g.nb, g.nb, red);
  if (tid == 0) {
    if (k == 0) g.ff[b] = rr;
    const double nf = sqrt(k == 0 ? rr : g.ff[b]), nr = sqrt(rr);
    g.iters[b] = k;
    g.resid[b] = nf > 0.0 ? nr / nf : 0.0;
    g.done[b] = nr <= rtol * nf ? 1 : 0;
  }
}

// init: x = 0, r = f, partial of f.f (into the r.r partials)
__global__ __launch_bounds__(kDivThreads) void div_init_kernel(const double* __restrict__ f, DivCG g) {
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  const long long base = (long long)b * n * n;
  const int gx = (int)blockIdx.x * kDivTX + (tid & 63);
  const int gy0 = (int)blockIdx.y * kDivTY + (tid >> 6) * kDivR;
  double acc = 0.0;
  if (gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int gy = gy0 + r;
      if (gy < n) {
        const long long at = base + (long long)gy * n + gx;
        const double fv = f[at];
        g.x[at] = 0.0;
        g.r[at] = fv;
        acc = acc + fv * fv;
      }
    }
  }
  const double s = block_sum(acc, red);
  if (tid == 0) g.prr[(size_t)b * g.nb + block_id()] = s;
}

// warm-started init: x = u0, r = f - D_theta u0 (D_theta u0 as div_apply_kernel forms it, then one subtraction) from
// the halo tiles of u0 and theta; the block's partials of f.f (into the p.q partials, free until iteration 1) and of
// r.r.  The walk and the sums are div_init_kernel's, so for u0 = 0 (D 0 = +0, f - 0 = f) both partials are its bits.
// SHIFT: r = f - (D_theta u0 - sigma * u0), the operator as div_apply_kernel<.., SHIFT> forms it (+0 for u0 = 0 too).
// BC: with the side mask bc (the body of div_init_from_kernel and div_init_from_bc_kernel).
// BD (with BC, of div_init_from_bd_kernel): r = f - A_bd u0 with the halo and the flux term of div_apply_tile<BD>; u0
// may be null (zeros: the same operations on 0.0); the first partial is of (f - b)^2, b = A_bd 0 at sigma = 0, i.e.
// b = face_ghost_sum * inv_h2, + bd_flux_sum * inv_h on a flux-side node, then the one subtraction f - b.
template <bool HARM, bool SHIFT, bool BC, bool BD = false>
__device__ __forceinline__ void div_init_from_tile(const double* __restrict__ f, const double* __restrict__ u0,
                                                   const double* __restrict__ theta, const DivCG& g, double inv_h2,
                                                   double sigma, int bc, const double* __restrict__ bd = nullptr,
                                                   double inv_h = 0.0) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  const long long base = (long long)b * n * n;
  const int x0 = (int)blockIdx.x * kDivTX, y0 = (int)blockIdx.y * kDivTY;
  for (int i = tid; i < kDivLY * kDivLX; i += kDivThreads) {
    const int ly = i / kDivLX, lx = i - ly * kDivLX;
    const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    double uv = 0.0, tv = 1.0;
    if (gy >= 0 && gy < n && gx >= 0 && gx < n) {
      const long long at = base + (long long)gy * n + gx;
      uv = (BD && !u0) ? 0.0 : u0[at];
      tv = theta[at];
    } else if (BD) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ts[i] = tv;
  }
  __syncthreads();

  const int lx = (tid & 63) + 1, gx = x0 + (tid & 63);
  const int ly0 = (tid >> 6) * kDivR + 1;
  double accf = 0.0, accr = 0.0;
  if (gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int ly = ly0 + r, gy = y0 + ly - 1;
      if (gy < n) {
        const int c = ly * kDivLX + lx;
        double du = node_face_sum<HARM, BC>(us, ts, c, gx, gy, n, bc) * inv_h2;
        double bv = 0.0;
        if (BD) {
          bv = face_ghost_sum(us + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n, !(bc & 4), !(bc & 8),
                              !(bc & 1), !(bc & 2)) * inv_h2;
          if (bd_flux_node(gy, gx, n, bc)) {
            const double q = bd_flux_sum(bd, gy, gx, n, bc) * inv_h;
            du = du + q;
            bv = bv + q;
          }
        }
        if (SHIFT) du = du - sigma * us[c];
        const long long at = base + (long long)gy * n + gx;
        double fv = f[at];
        const double rv = fv - du;
        g.x[at] = us[c];
        g.r[at] = rv;
        if (BD) fv = fv - bv;
        accf = accf + fv * fv;
        accr = accr + rv * rv;
      }
    }
  }
  const double sf = block_sum(accf, red);
  const double sr = block_sum(accr, red);
  if (tid == 0) {
    g.ppq[(size_t)b * g.nb + block_id()] = sf;
    g.prr[(size_t)b * g.nb + block_id()] = sr;
  }
}

template <bool HARM, bool SHIFT>
__global__ __launch_bounds__(kDivThreads) void div_init_from_kernel(const double* __restrict__ f,
                                                                    const double* __restrict__ u0,
                                                                    const double* __restrict__ theta, DivCG g,
                                                                    double inv_h2, double sigma) {
  div_init_from_tile<HARM, SHIFT, false>(f, u0, theta, g, inv_h2, sigma, 0);
}

template <bool HARM, bool SHIFT>
__global__ __launch_bounds__(kDivThreads) void div_init_from_bc_kernel(const double* __restrict__ f,
                                                                       const double* __restrict__ u0,
                                                                       const double* __restrict__ theta, DivCG g,
                                                                       double inv_h2, double sigma, int bc) {
  div_init_from_tile<HARM, SHIFT, true>(f, u0, theta, g, inv_h2, sigma, bc);
}

template <bool HARM, bool SHIFT>
__global__ __launch_bounds__(kDivThreads) void div_init_from_bd_kernel(const double* __restrict__ f,
                                                                       const double* __restrict__ u0,
                                                                       const double* __restrict__ theta, DivCG g,
                                                                       double inv_h2, double sigma, int bc,
                                                                       const double* __restrict__ bd,
                                                                       long long bd_stride, double inv_h) {
  div_init_from_tile<HARM, SHIFT, true, true>(f, u0, theta, g, inv_h2, sigma, bc,
                                              bd + (long long)blockIdx.z * bd_stride, inv_h);
}

// the k = 0 pass after div_init_from_kernel and the sine solve: the block's partial of r.z where iteration 1 reads
// it; |f|^2 from the p.q partials, |r0|^2 from the r.r partials; done at the caller's rtol, so a u0 that already
// satisfies it costs no iteration.  |f| = 0: every block zeroes its tile of x (u = 0 exactly, as the zero start).
__global__ __launch_bounds__(kDivThreads) void div_rz_from_kernel(DivCG g, double rtol) {
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  const long long base = (long long)b * n * n;
  const int gx = (int)blockIdx.x * kDivTX + (tid & 63);
  const int gy0 = (int)blockIdx.y * kDivTY + (tid >> 6) * kDivR;
  double acc = 0.0;
  if (gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int gy = gy0 + r;
      if (gy < n) {
        const long long at = base + (long long)gy * n + gx;
        acc = acc + g.r[at] * g.z[at];
      }
    }
  }
  const double s = block_sum(acc, red);
  if (tid == 0) g.prz[0][(size_t)b * g.nb + block_id()] = s;
  const double ff = resum(g.ppq + (size_t)b * g.nb, g.nb, red);
  if (ff == 0.0 && gx < n) {
#pragma unroll
    for (int r = 0; r < kDivR; ++r) {
      const int gy = gy0 + r;
      if (gy < n) g.x[base + (long long)gy * n + gx] = 0.0;
    }
  }
  if (block_id() != 0) return;
  const double rr = resum(g.prr + (size_t)b * g.nb, g.nb, red);
  if (tid == 0) {
    const double nf = sqrt(ff), nr = sqrt(rr);
    g.ff[b] = ff;
    g.iters[b] = 0;
    g.resid[b] = nf > 0.0 ? nr / nf : 0.0;
    g.done[b] = (ff == 0.0 || nr <= rtol * nf) ? 1 : 0;
  }
}

// The right-hand side of one implicit time step of u_t = D_theta u - f, for the solve (D_theta - sigma I) u+ = rhs:
//   CN false (backward Euler, sigma = 1 / dt):  rhs = f - sigma * u
//   CN true  (Crank-Nicolson, sigma = 2 / dt):  rhs = (2 f - sigma * u) - D_theta u
// 2 f is exact, D_theta u is div_apply_kernel's (face sum * inv_h2), every other operation is rounded once in the
// order written; f == nullptr is f = 0.  Backward Euler reads no neighbour and stages nothing in LDS.
// BC: with the side mask bc (the body of div_step_rhs_kernel and div_step_rhs_bc_kernel).
// BD (with BC and CN, of div_step_rhs_bd_kernel): A_bd u at sigma = 0 in place of D_theta u, as div_apply_tile<BD>.
template <bool CN, bool HARM, bool BC, bool BD = false>
__device__ __forceinline__ void div_step_rhs_tile(const double* __restrict__ u, const double* __restrict__ f,
                                                  const double* __restrict__ theta, double* __restrict__ rhs,
                                                  double inv_h2, double sigma, int n, int bc,
                                                  const double* __restrict__ bd = nullptr, double inv_h = 0.0) {
  __shared__ double us[CN ? kDivLY * kDivLX : 1];
  __shared__ double ts[CN ? kDivLY * kDivLX : 1];
  const int tid = threadIdx.x, b = blockIdx.z;
  const long long base = (long long)b * n * n;
  const int x0 = (int)blockIdx.x * kDivTX, y0 = (int)blockIdx.y * kDivTY;
  if (CN) {
    for (int i = tid; i < kDivLY * kDivLX; i += kDivThreads) {
      const int ly = i / kDivLX, lx = i - ly * kDivLX;
      const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
      double uv = 0.0, tv = 1.0;
      if (gy >= 0 && gy < n && gx >= 0 && gx < n) {
        const long long at = base + (long long)gy * n + gx;
        uv = u[at];
        tv = theta[at];
      } else if (BD) {
        uv = bd_halo(bd, gy, gx, n, bc);
      }
      us[i] = uv;
      ts[i] = tv;
    }
    __syncthreads();
  }

  const int lx = (tid & 63) + 1, gx = x0 + (tid & 63);
  const int ly0 = (tid >> 6) * kDivR + 1;
  if (gx >= n) return;
#pragma unroll
  for (int r = 0; r < kDivR; ++r) {
    const int ly = ly0 + r, gy = y0 + ly - 1;
    if (gy < n) {
      const long long at = base + (long long)gy * n + gx;
      const double fv = f ? f[at] : 0.0;
      if (CN) {
        const int c = ly * kDivLX + lx;
        double du = node_face_sum<HARM, BC>(us, ts, c, gx, gy, n, bc) * inv_h2;
        if (BD && bd_flux_node(gy, gx, n, bc)) du = du + bd_flux_sum(bd, gy, gx, n, bc) * inv_h;
        rhs[at] = (2.0 * fv - sigma * us[c]) - du;
      } else {
        rhs[at] = fv - sigma * u[at];
      }
    }
  }
}

template <bool CN, bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_step_rhs_kernel(const double* __restrict__ u,
                                                                   const double* __restrict__ f,
                                                                   const double* __restrict__ theta,
                                                                   double* __restrict__ rhs, double inv_h2,
                                                                   double sigma, int n) {
  div_step_rhs_tile<CN, HARM, false>(u, f, theta, rhs, inv_h2, sigma, n, 0);
}

// Crank-Nicolson only: backward Euler reads no neighbour, so a pattern changes nothing of it
template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_step_rhs_bc_kernel(const double* __restrict__ u,
                                                                      const double* __restrict__ f,
                                                                      const double* __restrict__ theta,
                                                                      double* __restrict__ rhs, double inv_h2,
                                                                      double sigma, int n, int bc) {
  div_step_rhs_tile<true, HARM, true>(u, f, theta, rhs, inv_h2, sigma, n, bc);
}

template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_step_rhs_bd_kernel(const double* __restrict__ u,
                                                                      const double* __restrict__ f,
                                                                      const double* __restrict__ theta,
                                                                      double* __restrict__ rhs, double inv_h2,
                                                                      double sigma, int n, int bc,
                                                                      const double* __restrict__ bd,
                                                                      long long bd_stride, double inv_h) {
  div_step_rhs_tile<true, HARM, true, true>(u, f, theta, rhs, inv_h2, sigma, n, bc,
                                            bd + (long long)blockIdx.z * bd_stride, inv_h);
}

// g = scale * G(u, lam; theta), G_a = inv_h2 * sum over a's faces of dc/dtheta_a (u_b - u_a) (lam_b - lam_a): the
// gradient in theta of <lam, D_theta u>.  A gather over the halo tiles of u, lam and theta (3 x 34 x 66 doubles of
// LDS, under the 64 KiB static limit): each node reads its own four faces, nothing is accumulated across nodes.
// BC: with the side mask bc (the body of div_theta_grad_kernel and div_theta_grad_bc_kernel).
// BD (with BC, of div_theta_grad_bd_kernel): u's out-of-grid halo holds g beyond Dirichlet sides, lam's stays 0, so a
// ghost face gives (1 * (g - u_a)) * (0 - lam_a); the prescribed flux does not depend on theta and adds nothing.
template <bool HARM, bool BC, bool BD = false>
__device__ __forceinline__ void div_theta_grad_tile(const double* __restrict__ u, const double* __restrict__ lam,
                                                    const double* __restrict__ theta, double* __restrict__ gout,
                                                    double inv_h2, double scale, int n, int bc,
                                                    const double* __restrict__ bd = nullptr) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ls[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  const int tid = threadIdx.x, b = blockIdx.z;
  const long long base = (long long)b * n * n;
  const int x0 = (int)blockIdx.x * kDivTX, y0 = (int)blockIdx.y * kDivTY;
  for (int i = tid; i < kDivLY * kDivLX; i += kDivThreads) {
    const int ly = i / kDivLX, lx = i - ly * kDivLX;
    const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    double uv = 0.0, lv = 0.0, tv = 1.0;
    if (gy >= 0 && gy < n && gx >= 0 && gx < n) {
      const long long at = base + (long long)gy * n + gx;
      uv = u[at];
      lv = lam[at];
      tv = theta[at];
    } else if (BD) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ls[i] = lv;
    ts[i] = tv;
  }
  __syncthreads();

  const int lx = (tid & 63) + 1, gx = x0 + (tid & 63);
  const int ly0 = (tid >> 6) * kDivR + 1;
  if (gx >= n) return;
#pragma unroll
  for (int r = 0; r < kDivR; ++r) {
    const int ly = ly0 + r, gy = y0 + ly - 1;
    if (gy < n) {
      const int c = ly * kDivLX + lx;
      const double gv = node_face_grad_sum<HARM, BC>(us, ls, ts, c, gx, gy, n, bc) * inv_h2;
      gout[base + (long long)gy * n + gx] = gv * scale;
    }
  }
}

template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_theta_grad_kernel(const double* __restrict__ u,
                                                                     const double* __restrict__ lam,
                                                                     const double* __restrict__ theta,
                                                                     double* __restrict__ gout, double inv_h2,
                                                                     double scale, int n) {
  div_theta_grad_tile<HARM, false>(u, lam, theta, gout, inv_h2, scale, n, 0);
}

template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_theta_grad_bc_kernel(const double* __restrict__ u,
                                                                        const double* __restrict__ lam,
                                                                        const double* __restrict__ theta,
                                                                        double* __restrict__ gout, double inv_h2,
                                                                        double scale, int n, int bc) {
  div_theta_grad_tile<HARM, true>(u, lam, theta, gout, inv_h2, scale, n, bc);
}

template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_theta_grad_bd_kernel(const double* __restrict__ u,
                                                                        const double* __restrict__ lam,
                                                                        const double* __restrict__ theta,
                                                                        double* __restrict__ gout, double inv_h2,
                                                                        double scale, int n, int bc,
                                                                        const double* __restrict__ bd,
                                                                        long long bd_stride) {
  div_theta_grad_tile<HARM, true, true>(u, lam, theta, gout, inv_h2, scale, n, bc,
                                        bd + (long long)blockIdx.z * bd_stride);
}

// out [B][4][n] = d<lam, A_bd u>/d bd: (inv_h2 * theta_a) * lam_a on a Dirichlet side, inv_h * lam_a on a flux side,
// a the side's edge node of entry k.  grid (ceil(n / 256), 4 sides, B): an edge gather, no node is shared.
__global__ __launch_bounds__(256) void div_bd_grad_kernel(const double* __restrict__ lam,
                                                          const double* __restrict__ theta, double* __restrict__ out,
                                                          int n, int bc, double inv_h2, double inv_h) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x, side = blockIdx.y, b = blockIdx.z;
  if (k >= n) return;
  const int gy = side == 0 ? 0 : (side == 1 ? n - 1 : k);
  const int gx = side == 2 ? 0 : (side == 3 ? n - 1 : k);
  const long long at = (long long)b * n * n + (long long)gy * n + gx;
  const double lv = lam[at];
  out[((long long)b * 4 + side) * n + k] = ((bc >> side) & 1) ? inv_h * lv : (inv_h2 * theta[at]) * lv;
}

__global__ __launch_bounds__(256) void div_finish_kernel(DivCG g, double* __restrict__ u, int* __restrict__ iters,
                                                         double* __restrict__ resid, long long total, int B) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    u[i] = g.x[i];
    if (i < B) {
      if (iters) iters[i] = g.iters[i];
      if (resid) resid[i] = g.resid[i];
    }
  }
}

inline dim3 div_grid(int B, int n) { return dim3(ceil_div(n, kDivTX), ceil_div(n, kDivTY), B); }

}  // namespace
}  // namespace srpde

using namespace srpde;

static int div_check(const char* name, int B, int n, int face_mean) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN)
    SRPDE_FAIL(kErrShape, "%s: bad shape B=%d n=%d (1 <= B <= %d, 2 <= n <= %d)", name, B, n, kDivMaxB, kDivMaxN);
  if (face_mean != 0 && face_mean != 1)
    SRPDE_FAIL(kErrArg, "%s: face_mean=%d (0 arithmetic, 1 harmonic)", name, face_mean);
  return 0;
}

static int div_check_ws(const char* name, int B, int n, const void* ws, size_t ws_bytes, bool bc = false) {
  if (!ws) SRPDE_FAIL(kErrArg, "%s: null workspace", name);
  if (!aligned16(ws)) SRPDE_FAIL(kErrAlign, "%s: workspace not 16-byte aligned", name);
  const size_t need = bc ? srpde_div_cg_workspace_size_bc(B, n) : srpde_div_cg_workspace_size(B, n);
  if (ws_bytes < need) SRPDE_FAIL(kErrWorkspace, "%s: workspace too small (%zu bytes, needs %zu)", name, ws_bytes, need);
  return 0;
}

// bc < 0: the sine-transform plan for n; else the separable plan for n and that side mask
static int div_check_plan(const char* name, int n, const void* plan, size_t plan_bytes, int bc = -1) {
  if (!plan) SRPDE_FAIL(kErrArg, "%s: null plan", name);
  if (reinterpret_cast<uintptr_t>(plan) & 7u) SRPDE_FAIL(kErrAlign, "%s: plan not 8-byte aligned", name);
  if (bc >= 0) {
    if (plan_bytes != sep_plan_bytes_for(n, bc))
      SRPDE_FAIL(kErrWorkspace, "%s: a plan of %zu bytes is not a plan for n=%d and bc=%d (srpde_poisson_sep_plan_size: %zu)",
                 name, plan_bytes, n, bc, sep_plan_bytes_for(n, bc));
    return 0;
  }
  if (plan_bytes != dst_plan_bytes_for(n))
    SRPDE_FAIL(kErrWorkspace, "%s: a plan of %zu bytes is not a plan for n=%d (srpde_poisson_dst_plan_size: %zu)", name,
               plan_bytes, n, dst_plan_bytes_for(n));
  return 0;
}

// the side mask of a *_bc entry; all four sides zero-flux is singular without a shift
static int div_check_bc(const char* name, int bc) {
  if (bc < 0 || bc > 15)
    SRPDE_FAIL(kErrArg, "%s: bc=%d is not a side mask (bits 0..3: row 0, row n-1, column 0, column n-1; set = zero flux)",
               name, bc);
  return 0;
}

static int div_check_singular(const char* name, int bc, const char* what, double sigma) {
  if (bc == 15 && sigma == 0.0)
    SRPDE_FAIL(kErrArg, "%s: four zero-flux sides (bc=15) with %s=0 is singular (the constants): it needs a shift > 0",
               name, what);
  return 0;
}

// step (c): z = M^-1 r -- the sine-transform solve (bc < 0), or the separable solve with that side mask
static int div_precondition(const char* name, const DivCG& g, int B, int n, int bc, const void* plan,
                            hipStream_t stream, double sigma_p) {
  if (bc < 0) return dst_solve_launch(name, g.r, nullptr, g.z, B, n, plan, g.dst_ws, stream, sigma_p);
  return sep_solve_launch(name, g.r, g.z, B, n, plan, g.sep_ws, stream, sigma_p);
}

extern "C" {

size_t srpde_div_cg_workspace_size_bc(int B, int n) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN) return 0;
  return carve(nullptr, B, n, true).bytes;
}

size_t srpde_div_cg_workspace_size(int B, int n) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN) return 0;
  return carve(nullptr, B, n).bytes;
}

size_t srpde_div_cg_done_offset(int B, int n) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN) return 0;
  return (size_t)(reinterpret_cast<char*>(carve(nullptr, B, n).done) - static_cast<char*>(nullptr));
}

// sigma >= 0 and finite; the message names the entry
static int div_check_sigma(const char* name, const char* what, double sigma) {
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) SRPDE_FAIL(kErrArg, "%s: %s=%g must be >= 0 and finite", name, what, sigma);
  return 0;
}

// srpde_div_apply, srpde_div_apply_shift and srpde_div_apply_bc (bc >= 0): sigma = 0 is the unshifted kernel
static int div_apply_launch(const char* name, const double* u, const double* theta, double* y, int B, int n,
                            int face_mean, double inv_h2, double sigma, hipStream_t stream, int bc = -1) {
  SRPDE_CHECK_ARG(u && theta && y, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (bc != -1)
    if (int rc = div_check_bc(name, bc)) return rc;
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(y)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (y == u || y == theta) SRPDE_FAIL(kErrArg, "%s: y aliases an input (a node reads its neighbours)", name);
  DivCG none = {};
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  if (bc >= 0) {
    switch ((sigma != 0.0 ? 2 : 0) + (face_mean ? 1 : 0)) {
      case 0:
        hipLaunchKernelGGL((div_apply_bc_kernel<false, false, false>), grid, block, 0, stream, u, theta, y, none, inv_h2,
                           0.0, n, 0, bc);
        break;
      case 1:
        hipLaunchKernelGGL((div_apply_bc_kernel<false, true, false>), grid, block, 0, stream, u, theta, y, none, inv_h2,
                           0.0, n, 0, bc);
        break;
      case 2:
        hipLaunchKernelGGL((div_apply_bc_kernel<false, false, true>), grid, block, 0, stream, u, theta, y, none, inv_h2,
                           sigma, n, 0, bc);
        break;
      default:
        hipLaunchKernelGGL((div_apply_bc_kernel<false, true, true>), grid, block, 0, stream, u, theta, y, none, inv_h2,
                           sigma, n, 0, bc);
    }
  } else if (sigma != 0.0) {
    if (face_mean)
      hipLaunchKernelGGL((div_apply_kernel<false, true, true>), grid, block, 0, stream, u, theta, y, none, inv_h2,
                         sigma, n, 0);
    else
      hipLaunchKernelGGL((div_apply_kernel<false, false, true>), grid, block, 0, stream, u, theta, y, none, inv_h2,
                         sigma, n, 0);
  } else if (face_mean) {
    hipLaunchKernelGGL((div_apply_kernel<false, true, false>), grid, block, 0, stream, u, theta, y, none, inv_h2, 0.0,
                       n, 0);
  } else {
    hipLaunchKernelGGL((div_apply_kernel<false, false, false>), grid, block, 0, stream, u, theta, y, none, inv_h2, 0.0,
                       n, 0);
  }
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_apply(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                    hipStream_t stream) {
  return div_apply_launch("srpde_div_apply", u, theta, y, B, n, face_mean, inv_h2, 0.0, stream);
}

int srpde_div_apply_shift(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                          double sigma, hipStream_t stream) {
  return div_apply_launch("srpde_div_apply_shift", u, theta, y, B, n, face_mean, inv_h2, sigma, stream);
}

int srpde_div_apply_bc(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                       double sigma, int bc, hipStream_t stream) {
  return div_apply_launch("srpde_div_apply_bc", u, theta, y, B, n, face_mean, inv_h2, sigma, stream, bc < 0 ? 16 : bc);
}

// srpde_div_step_rhs and srpde_div_step_rhs_bc (bc >= 0)
static int div_step_rhs(const char* name, const double* u, const double* f, const double* theta, double* rhs, int B,
                        int n, int face_mean, double sigma, int cn, int bc, hipStream_t stream) {
  SRPDE_CHECK_ARG(u && theta && rhs, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (bc != -1)
    if (int rc = div_check_bc(name, bc)) return rc;
  if (cn != 0 && cn != 1) SRPDE_FAIL(kErrArg, "%s: cn=%d (0 backward Euler, 1 Crank-Nicolson)", name, cn);
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(theta) |
       reinterpret_cast<uintptr_t>(rhs)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (rhs == u || rhs == theta || rhs == f)
    SRPDE_FAIL(kErrArg, "%s: rhs aliases an input (a node reads its neighbours)", name);
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  if (cn && bc >= 0) {
    if (face_mean)
      hipLaunchKernelGGL(div_step_rhs_bc_kernel<true>, grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n, bc);
    else
      hipLaunchKernelGGL(div_step_rhs_bc_kernel<false>, grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n, bc);
  } else if (!cn)
    hipLaunchKernelGGL((div_step_rhs_kernel<false, false>), grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n);
  else if (face_mean)
    hipLaunchKernelGGL((div_step_rhs_kernel<true, true>), grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n);
  else
    hipLaunchKernelGGL((div_step_rhs_kernel<true, false>), grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_step_rhs(const double* u, const double* f, const double* theta, double* rhs, int B, int n, int face_mean,
                       double sigma, int cn, hipStream_t stream) {
  return div_step_rhs("srpde_div_step_rhs", u, f, theta, rhs, B, n, face_mean, sigma, cn, -1, stream);
}

int srpde_div_step_rhs_bc(const double* u, const double* f, const double* theta, double* rhs, int B, int n,
                          int face_mean, double sigma, int cn, int bc, hipStream_t stream) {
  return div_step_rhs("srpde_div_step_rhs_bc", u, f, theta, rhs, B, n, face_mean, sigma, cn, bc < 0 ? 16 : bc, stream);
}

// srpde_div_cg_init and srpde_div_cg_init_shift (the zero start has r = f whatever sigma is: only M changes)
static int div_cg_init(const char* name, const double* f, int B, int n, double sigma_p, const void* plan,
                       size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream, int bc = -1) {
  SRPDE_CHECK_ARG(f, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, 0)) return rc;
  if (bc != -1)
    if (int rc = div_check_bc(name, bc)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma_p", sigma_p)) return rc;
  if (reinterpret_cast<uintptr_t>(f) & 7u) SRPDE_FAIL(kErrAlign, "%s: f not 8-byte aligned", name);
  if (int rc = div_check_plan(name, n, plan, plan_bytes, bc)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, bc >= 0)) return rc;
  DivCG g = carve(ws, B, n, bc >= 0);
  hipLaunchKernelGGL(div_init_kernel, div_grid(B, n), dim3(kDivThreads), 0, stream, f, g);
  SRPDE_LAUNCH_CHECK(name);
  if (int rc = div_precondition(name, g, B, n, bc, plan, stream, sigma_p)) return rc;
  // rtol 0: only |f| = 0 is done before the first iteration
  hipLaunchKernelGGL(div_rz_kernel, div_grid(B, n), dim3(kDivThreads), 0, stream, g, 0, 0.0);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_cg_init(const double* f, int B, int n, const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                      hipStream_t stream) {
  return div_cg_init("srpde_div_cg_init", f, B, n, 0.0, plan, plan_bytes, ws, ws_bytes, stream);
}

int srpde_div_cg_init_shift(const double* f, int B, int n, double sigma_p, const void* plan, size_t plan_bytes,
                            void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init("srpde_div_cg_init_shift", f, B, n, sigma_p, plan, plan_bytes, ws, ws_bytes, stream);
}

static int div_cg_init_from(const char* name, const double* f, const double* u0, const double* theta, int B, int n,
                            int face_mean, double sigma, double sigma_p, double rtol, const void* plan,
                            size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream, int bc = -1) {
  SRPDE_CHECK_ARG(f && u0 && theta, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (bc != -1)
    if (int rc = div_check_bc(name, bc)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma", sigma)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma_p", sigma_p)) return rc;
  if ((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(u0) | reinterpret_cast<uintptr_t>(theta)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (!(rtol >= 0.0)) SRPDE_FAIL(kErrArg, "%s: rtol=%g must be >= 0", name, rtol);
  if (int rc = div_check_plan(name, n, plan, plan_bytes, bc)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, bc >= 0)) return rc;
  DivCG g = carve(ws, B, n, bc >= 0);
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  if (bc >= 0) {
    switch ((sigma != 0.0 ? 2 : 0) + (face_mean ? 1 : 0)) {
      case 0:
        hipLaunchKernelGGL((div_init_from_bc_kernel<false, false>), grid, block, 0, stream, f, u0, theta, g, inv_h2, 0.0,
                           bc);
        break;
      case 1:
        hipLaunchKernelGGL((div_init_from_bc_kernel<true, false>), grid, block, 0, stream, f, u0, theta, g, inv_h2, 0.0,
                           bc);
        break;
      case 2:
        hipLaunchKernelGGL((div_init_from_bc_kernel<false, true>), grid, block, 0, stream, f, u0, theta, g, inv_h2,
                           sigma, bc);
        break;
      default:
        hipLaunchKernelGGL((div_init_from_bc_kernel<true, true>), grid, block, 0, stream, f, u0, theta, g, inv_h2, sigma,
                           bc);
    }
  } else if (sigma != 0.0) {
    if (face_mean)
      hipLaunchKernelGGL((div_init_from_kernel<true, true>), grid, block, 0, stream, f, u0, theta, g, inv_h2, sigma);
    else
      hipLaunchKernelGGL((div_init_from_kernel<false, true>), grid, block, 0, stream, f, u0, theta, g, inv_h2, sigma);
  } else if (face_mean) {
    hipLaunchKernelGGL((div_init_from_kernel<true, false>), grid, block, 0, stream, f, u0, theta, g, inv_h2, 0.0);
  } else {
    hipLaunchKernelGGL((div_init_from_kernel<false, false>), grid, block, 0, stream, f, u0, theta, g, inv_h2, 0.0);
  }
  SRPDE_LAUNCH_CHECK(name);
  if (int rc = div_precondition(name, g, B, n, bc, plan, stream, sigma_p)) return rc;
  hipLaunchKernelGGL(div_rz_from_kernel, grid, block, 0, stream, g, rtol);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_cg_init_from(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                           double rtol, const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                           hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from", f, u0, theta, B, n, face_mean, 0.0, 0.0, rtol, plan, plan_bytes,
                          ws, ws_bytes, stream);
}

int srpde_div_cg_init_from_shift(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                                 double sigma, double sigma_p, double rtol, const void* plan, size_t plan_bytes,
                                 void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from_shift", f, u0, theta, B, n, face_mean, sigma, sigma_p, rtol, plan,
                          plan_bytes, ws, ws_bytes, stream);
}

// srpde_div_theta_grad and srpde_div_theta_grad_bc (bc >= 0)
static int div_theta_grad(const char* name, const double* u, const double* lam, const double* theta, double* g_out,
                          int B, int n, int face_mean, double inv_h2, double scale, int bc, hipStream_t stream) {
  SRPDE_CHECK_ARG(u && lam && theta && g_out, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (bc != -1)
    if (int rc = div_check_bc(name, bc)) return rc;
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  if (!std::isfinite(scale)) SRPDE_FAIL(kErrArg, "%s: scale=%g must be finite", name, scale);
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(lam) | reinterpret_cast<uintptr_t>(theta) |
       reinterpret_cast<uintptr_t>(g_out)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (g_out == u || g_out == lam || g_out == theta)
    SRPDE_FAIL(kErrArg, "%s: g_out aliases an input (a node reads its neighbours)", name);
  if (bc >= 0 && face_mean)
    hipLaunchKernelGGL(div_theta_grad_bc_kernel<true>, div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam, theta,
                       g_out, inv_h2, scale, n, bc);
  else if (bc >= 0)
    hipLaunchKernelGGL(div_theta_grad_bc_kernel<false>, div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam, theta,
                       g_out, inv_h2, scale, n, bc);
  else if (face_mean)
    hipLaunchKernelGGL(div_theta_grad_kernel<true>, div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam, theta, g_out,
                       inv_h2, scale, n);
  else
    hipLaunchKernelGGL(div_theta_grad_kernel<false>, div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam, theta,
                       g_out, inv_h2, scale, n);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_theta_grad(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                         int face_mean, double inv_h2, double scale, hipStream_t stream) {
  return div_theta_grad("srpde_div_theta_grad", u, lam, theta, g_out, B, n, face_mean, inv_h2, scale, -1, stream);
}

int srpde_div_theta_grad_bc(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                            int face_mean, double inv_h2, double scale, int bc, hipStream_t stream) {
  return div_theta_grad("srpde_div_theta_grad_bc", u, lam, theta, g_out, B, n, face_mean, inv_h2, scale,
                        bc < 0 ? 16 : bc, stream);
}

static int div_cg_iterate(const char* name, const double* theta, int B, int n, int face_mean, double sigma,
                          double sigma_p, double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes,
                          void* ws, size_t ws_bytes, hipStream_t stream, int bc = -1) {
  SRPDE_CHECK_ARG(theta, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (bc != -1)
    if (int rc = div_check_bc(name, bc)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma", sigma)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma_p", sigma_p)) return rc;
  if (reinterpret_cast<uintptr_t>(theta) & 7u) SRPDE_FAIL(kErrAlign, "%s: theta not 8-byte aligned", name);
  if (!(rtol >= 0.0)) SRPDE_FAIL(kErrArg, "%s: rtol=%g must be >= 0", name, rtol);
  if (k_begin < 1 || k_count < 0 || k_count > INT32_MAX - k_begin)
    SRPDE_FAIL(kErrArg, "%s: k_begin=%d k_count=%d (iterations count from 1)", name, k_begin, k_count);
  if (int rc = div_check_plan(name, n, plan, plan_bytes, bc)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, bc >= 0)) return rc;
  DivCG g = carve(ws, B, n, bc >= 0);
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  const int variant = (bc >= 0 ? 4 : 0) + (sigma != 0.0 ? 2 : 0) + (face_mean ? 1 : 0);
  for (int k = k_begin; k < k_begin + k_count; ++k) {
    switch (variant) {
      case 4:
        hipLaunchKernelGGL((div_apply_bc_kernel<true, false, false>), grid, block, 0, stream, g.z, theta, g.q, g,
                           inv_h2, 0.0, n, k, bc);
        break;
      case 5:
        hipLaunchKernelGGL((div_apply_bc_kernel<true, true, false>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           0.0, n, k, bc);
        break;
      case 6:
        hipLaunchKernelGGL((div_apply_bc_kernel<true, false, true>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           sigma, n, k, bc);
        break;
      case 7:
        hipLaunchKernelGGL((div_apply_bc_kernel<true, true, true>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           sigma, n, k, bc);
        break;
      case 0:
        hipLaunchKernelGGL((div_apply_kernel<true, false, false>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           0.0, n, k);
        break;
      case 1:
        hipLaunchKernelGGL((div_apply_kernel<true, true, false>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           0.0, n, k);
        break;
      case 2:
        hipLaunchKernelGGL((div_apply_kernel<true, false, true>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           sigma, n, k);
        break;
      default:
        hipLaunchKernelGGL((div_apply_kernel<true, true, true>), grid, block, 0, stream, g.z, theta, g.q, g, inv_h2,
                           sigma, n, k);
    }
    hipLaunchKernelGGL(div_update_kernel, grid, block, 0, stream, g, k);
    SRPDE_LAUNCH_CHECK(name);
    if (int rc = div_precondition(name, g, B, n, bc, plan, stream, sigma_p)) return rc;
    hipLaunchKernelGGL(div_rz_kernel, grid, block, 0, stream, g, k, rtol);
    SRPDE_LAUNCH_CHECK(name);
  }
  return 0;
}

int srpde_div_cg_iterate(const double* theta, int B, int n, int face_mean, double rtol, int k_begin, int k_count,
                         const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_iterate("srpde_div_cg_iterate", theta, B, n, face_mean, 0.0, 0.0, rtol, k_begin, k_count, plan,
                        plan_bytes, ws, ws_bytes, stream);
}

int srpde_div_cg_iterate_shift(const double* theta, int B, int n, int face_mean, double sigma, double sigma_p,
                               double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes, void* ws,
                               size_t ws_bytes, hipStream_t stream) {
  return div_cg_iterate("srpde_div_cg_iterate_shift", theta, B, n, face_mean, sigma, sigma_p, rtol, k_begin, k_count,
                        plan, plan_bytes, ws, ws_bytes, stream);
}

int srpde_div_cg_init_bc(const double* f, int B, int n, int bc, double sigma_p, const void* plan, size_t plan_bytes,
                         void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init("srpde_div_cg_init_bc", f, B, n, sigma_p, plan, plan_bytes, ws, ws_bytes, stream,
                     bc < 0 ? 16 : bc);
}

int srpde_div_cg_init_from_bc(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                              int bc, double sigma, double sigma_p, double rtol, const void* plan, size_t plan_bytes,
                              void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from_bc", f, u0, theta, B, n, face_mean, sigma, sigma_p, rtol, plan,
                          plan_bytes, ws, ws_bytes, stream, bc < 0 ? 16 : bc);
}

int srpde_div_cg_iterate_bc(const double* theta, int B, int n, int face_mean, int bc, double sigma, double sigma_p,
                            double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes, void* ws,
                            size_t ws_bytes, hipStream_t stream) {
  return div_cg_iterate("srpde_div_cg_iterate_bc", theta, B, n, face_mean, sigma, sigma_p, rtol, k_begin, k_count,
                        plan, plan_bytes, ws, ws_bytes, stream, bc < 0 ? 16 : bc);
}

// ---- boundary data (the *_bd entries): the side mask 0 .. 15 (0: four Dirichlet sides with values), bd [Bd][4][n]
static int div_check_bd(const char* name, int n, int bc, const double* bd, long long bd_stride) {
  if (int rc = div_check_bc(name, bc < 0 ? 16 : bc)) return rc;
  if (!bd) SRPDE_FAIL(kErrArg, "%s: null boundary data", name);
  if (reinterpret_cast<uintptr_t>(bd) & 7u) SRPDE_FAIL(kErrAlign, "%s: bd not 8-byte aligned", name);
  if (bd_stride != 0 && bd_stride != 4LL * n)
    SRPDE_FAIL(kErrArg, "%s: bd_stride=%lld is neither 4 n = %lld ([B][4][n]) nor 0 (one [4][n] for every problem)", name,
               bd_stride, 4LL * n);
  return 0;
}

int srpde_div_apply_bd(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                       double sigma, int bc, const double* bd, long long bd_stride, hipStream_t stream) {
  const char* name = "srpde_div_apply_bd";
  SRPDE_CHECK_ARG(u && theta && y, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_bd(name, n, bc, bd, bd_stride)) return rc;
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(y)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (y == u || y == theta || y == bd) SRPDE_FAIL(kErrArg, "%s: y aliases an input (a node reads its neighbours)", name);
  const double inv_h = std::sqrt(inv_h2);
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  switch ((sigma != 0.0 ? 2 : 0) + (face_mean ? 1 : 0)) {
    case 0:
      hipLaunchKernelGGL((div_apply_bd_kernel<false, false>), grid, block, 0, stream, u, theta, y, inv_h2, 0.0, n, bc,
                         bd, bd_stride, inv_h);
      break;
    case 1:
      hipLaunchKernelGGL((div_apply_bd_kernel<true, false>), grid, block, 0, stream, u, theta, y, inv_h2, 0.0, n, bc,
                         bd, bd_stride, inv_h);
      break;
    case 2:
      hipLaunchKernelGGL((div_apply_bd_kernel<false, true>), grid, block, 0, stream, u, theta, y, inv_h2, sigma, n, bc,
                         bd, bd_stride, inv_h);
      break;
    default:
      hipLaunchKernelGGL((div_apply_bd_kernel<true, true>), grid, block, 0, stream, u, theta, y, inv_h2, sigma, n, bc,
                         bd, bd_stride, inv_h);
  }
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_step_rhs_bd(const double* u, const double* f, const double* theta, double* rhs, int B, int n,
                          int face_mean, double sigma, int cn, int bc, const double* bd, long long bd_stride,
                          hipStream_t stream) {
  const char* name = "srpde_div_step_rhs_bd";
  if (int rc = div_check_bd(name, n, bc, bd, bd_stride)) return rc;
  // backward Euler reads no neighbour, so no data either: srpde_div_step_rhs_bc's checks and launch
  if (cn != 1) return div_step_rhs(name, u, f, theta, rhs, B, n, face_mean, sigma, cn, bc, stream);
  SRPDE_CHECK_ARG(u && theta && rhs, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(theta) |
       reinterpret_cast<uintptr_t>(rhs)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (rhs == u || rhs == theta || rhs == f || rhs == bd)
    SRPDE_FAIL(kErrArg, "%s: rhs aliases an input (a node reads its neighbours)", name);
  const double inv_h = (double)(n - 1), inv_h2 = inv_h * inv_h;
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  if (face_mean)
    hipLaunchKernelGGL(div_step_rhs_bd_kernel<true>, grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n, bc, bd,
                       bd_stride, inv_h);
  else
    hipLaunchKernelGGL(div_step_rhs_bd_kernel<false>, grid, block, 0, stream, u, f, theta, rhs, inv_h2, sigma, n, bc, bd,
                       bd_stride, inv_h);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_cg_init_from_bd(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                              int bc, double sigma, double sigma_p, double rtol, const double* bd, long long bd_stride,
                              const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  const char* name = "srpde_div_cg_init_from_bd";
  SRPDE_CHECK_ARG(f && theta, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_bd(name, n, bc, bd, bd_stride)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma", sigma)) return rc;
  if (int rc = div_check_singular(name, bc, "sigma_p", sigma_p)) return rc;
  if ((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(u0) | reinterpret_cast<uintptr_t>(theta)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (!(rtol >= 0.0)) SRPDE_FAIL(kErrArg, "%s: rtol=%g must be >= 0", name, rtol);
  // mask 0: the sine plan and the workspace of srpde_div_cg_workspace_size; else the separable plan and the _bc one
  const int pbc = bc ? bc : -1;
  if (int rc = div_check_plan(name, n, plan, plan_bytes, pbc)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, bc != 0)) return rc;
  DivCG g = carve(ws, B, n, bc != 0);
  const double inv_h = (double)(n - 1), inv_h2 = inv_h * inv_h;
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  switch ((sigma != 0.0 ? 2 : 0) + (face_mean ? 1 : 0)) {
    case 0:
      hipLaunchKernelGGL((div_init_from_bd_kernel<false, false>), grid, block, 0, stream, f, u0, theta, g, inv_h2, 0.0,
                         bc, bd, bd_stride, inv_h);
      break;
    case 1:
      hipLaunchKernelGGL((div_init_from_bd_kernel<true, false>), grid, block, 0, stream, f, u0, theta, g, inv_h2, 0.0,
                         bc, bd, bd_stride, inv_h);
      break;
    case 2:
      hipLaunchKernelGGL((div_init_from_bd_kernel<false, true>), grid, block, 0, stream, f, u0, theta, g, inv_h2, sigma,
                         bc, bd, bd_stride, inv_h);
      break;
    default:
      hipLaunchKernelGGL((div_init_from_bd_kernel<true, true>), grid, block, 0, stream, f, u0, theta, g, inv_h2, sigma,
                         bc, bd, bd_stride, inv_h);
  }
  SRPDE_LAUNCH_CHECK(name);
  if (int rc = div_precondition(name, g, B, n, pbc, plan, stream, sigma_p)) return rc;
  hipLaunchKernelGGL(div_rz_from_kernel, grid, block, 0, stream, g, rtol);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_theta_grad_bd(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                            int face_mean, double inv_h2, double scale, int bc, const double* bd, long long bd_stride,
                            hipStream_t stream) {
  const char* name = "srpde_div_theta_grad_bd";
  SRPDE_CHECK_ARG(u && lam && theta && g_out, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_bd(name, n, bc, bd, bd_stride)) return rc;
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  if (!std::isfinite(scale)) SRPDE_FAIL(kErrArg, "%s: scale=%g must be finite", name, scale);
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(lam) | reinterpret_cast<uintptr_t>(theta) |
       reinterpret_cast<uintptr_t>(g_out)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (g_out == u || g_out == lam || g_out == theta || g_out == bd)
    SRPDE_FAIL(kErrArg, "%s: g_out aliases an input (a node reads its neighbours)", name);
  if (face_mean)
    hipLaunchKernelGGL(div_theta_grad_bd_kernel<true>, div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam, theta,
                       g_out, inv_h2, scale, n, bc, bd, bd_stride);
  else
    hipLaunchKernelGGL(div_theta_grad_bd_kernel<false>, div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam, theta,
                       g_out, inv_h2, scale, n, bc, bd, bd_stride);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_bd_grad(const double* lam, const double* theta, double* out, int B, int n, double inv_h2, int bc,
                      hipStream_t stream) {
  const char* name = "srpde_div_bd_grad";
  SRPDE_CHECK_ARG(lam && theta && out, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, 0)) return rc;
  if (int rc = div_check_bc(name, bc < 0 ? 16 : bc)) return rc;
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  if ((reinterpret_cast<uintptr_t>(lam) | reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(out)) & 7u)
    SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (out == lam || out == theta) SRPDE_FAIL(kErrArg, "%s: out aliases an input", name);
  hipLaunchKernelGGL(div_bd_grad_kernel, dim3(ceil_div(n, 256), 4, B), dim3(256), 0, stream, lam, theta, out, n, bc,
                     inv_h2, std::sqrt(inv_h2));
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_cg_finish(double* u, int* iters, double* resid, int B, int n, void* ws, size_t ws_bytes,
                        hipStream_t stream) {
  const char* name = "srpde_div_cg_finish";
  SRPDE_CHECK_ARG(u, "srpde_div_cg_finish: null pointer");
  if (int rc = div_check(name, B, n, 0)) return rc;
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(resid)) & 7u)
    SRPDE_FAIL(kErrAlign, "srpde_div_cg_finish: a pointer is not 8-byte aligned");
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes)) return rc;
  DivCG g = carve(ws, B, n);
  const long long total = (long long)B * n * n;
  hipLaunchKernelGGL(div_finish_kernel, dim3(elementwise_grid(total)), dim3(256), 0, stream, g, u, iters, resid, total,
                     B);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

}  // extern "C"
