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
// Sides.  What lies beyond the grid's four sides is one descriptor, DivSides, which every entry builds and every helper
// and tile kernel takes; its kind is the kernels' last template argument:
//   Sides::kRing  the zero ghost ring above (the entries without a suffix and the *_shift entries)
//   Sides::kMask  a boundary pattern (the *_bc entries).  bc is a 4-bit mask, bit 0 the row 0 side, bit 1 the row n - 1
//                 side, bit 2 the column 0 side, bit 3 the column n - 1 side; a set bit is a zero-flux side: its ghost
//                 faces are missing (coefficient 0), a clear bit is the zero ghost ring.  The operator stays a sum over
//                 faces with c in [theta_min, theta_max], and so does M = L_bc - sigma_p I, the constant-coefficient
//                 operator with the same sides, which poisson_dst.hip's separable solve inverts exactly: cond(M^-1 A)
//                 <= theta_max / theta_min for every n, sigma and pattern.  All four sides zero-flux with sigma = 0 is
//                 singular (the constants) and refused.  Step (c) is the separable solve; update, r.z, the k = 0 pass,
//                 the freeze rule and finish are the code above, untouched.
//   Sides::kData  a pattern with boundary data (the *_bd entries).  bd [Bd][4][n] gives the sides values: the ghost
//                 value g beyond a Dirichlet side's edge node, the outward flux q through a zero-flux side's ghost face
//                 (div_stencil.h).  A_bd u = D_bc u - sigma u + b: the kernels stage g into the out-of-grid halo of u
//                 (bd_halo, reached only by entries outside the grid) and add ((qE + qW) + (qS + qN)) * inv_h at
//                 flux-side nodes after the face sum's * inv_h2.  The solve is (D_bc - sigma I) u = f - b:
//                 srpde_div_cg_init_from_bd forms r = f - A_bd u0 and the partials of (f - b)^2, the stop rule's
//                 reference, in one pass, and the iteration above runs unchanged, without data.
// A mask takes the separable plan and the workspace of srpde_div_cg_workspace_size_bc; the ring, and data with mask 0,
// take the sine plan and the workspace of srpde_div_cg_workspace_size (separable()).  div_dispatch turns the kind, the
// shift and the face mean into the template arguments of the one launch statement each launcher has.
//
// Adjoint (srpde_div_theta_grad).  D_theta is symmetric, so the adjoint of the solve is the same solve, and the
// gradient in theta of <lam, D_theta u> is the local pair gradient G(u, lam; theta) of div_theta_grad_kernel.
//
// Fluxes (srpde_div_face_flux, srpde_div_wall_flux and their _grad).  theta du/dx and theta du/dy on the faces, whose
// difference quotient is A_bd u, from the same halo tiles; their integral over each wall from the edge nodes alone, in
// one fixed order; both adjoints as gathers.  They read the state and change nothing of the solver.
#include <cmath>
#include <initializer_list>
#include <type_traits>

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

// what lies beyond the four sides (header, Sides).  bc: the mask as the caller gave it (0 for the ring); bd, bd_stride
// (4 n, or 0 for one [4][n] shared by every problem) and inv_h: of kData only
enum class Sides { kRing, kMask, kData };
struct DivSides {
  Sides kind;
  int bc;
  const double* bd;
  long long bd_stride;
  double inv_h;
};

inline DivSides ring_sides() { return {Sides::kRing, 0, nullptr, 0, 0.0}; }
inline DivSides mask_sides(int bc) { return {Sides::kMask, bc, nullptr, 0, 0.0}; }
inline DivSides data_sides(int bc, const double* bd, long long bd_stride, double inv_h) {
  return {Sides::kData, bc, bd, bd_stride, inv_h};
}

// the separable plan, its solve and the *_bc workspace layout; else the sine plan, its solve and the plain layout
inline bool separable(const DivSides& s) { return s.kind == Sides::kMask || (s.kind == Sides::kData && s.bc != 0); }

struct DivCG {
  double *x, *r, *z, *q, *p[2];            // [B][n][n]
  double *prr, *ppq, *prz[2];              // [B][nb] per-block partials
  double *ff, *resid;                      // [B]
  int *iters, *done;                       // [B]
  void* dst_ws;
  void* sep_ws;                            // the separable solve's field (carve with separable sides only)
  int n, nb;
  size_t bytes;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// separable sides: the layout of the *_bc entries -- the same offsets, so srpde_div_cg_finish and the done flags serve
// both, plus the separable solve's [B][n][n] field at the end where the sine solve's workspace is empty (n up to its
// LDS limit)
DivCG carve(void* ws, int B, int n, const DivSides& s) {
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
  if (separable(s) && srpde_poisson_dst_workspace_size(B, n) == 0) g.sep_ws = take(field);
  g.bytes = at;
  return g;
}

// block_sum and resum (field_reduce.h) give the same bits in every thread.  red, their 4 doubles of LDS, is used for
// nothing else in these kernels, and each call's first barrier comes before its write, so back-to-back calls are safe.

__device__ __forceinline__ int block_id() { return (int)(blockIdx.y * gridDim.x + blockIdx.x); }

// Halo staging: put(i, in, at, gy, gx) for every entry i of the block's 34 x 66 halo tiles, (gy, gx) its grid position,
// in: that is a node of the grid, at: the node's address then.  put writes entry i of every tile the kernel stages.
// The callables of both walks capture by value, and by reference only the sums they add to.
template <class Put>
__device__ __forceinline__ void div_halo_walk(long long base, int n, Put put) {
  const int x0 = (int)blockIdx.x * kDivTX, y0 = (int)blockIdx.y * kDivTY;
  for (int i = threadIdx.x; i < kDivLY * kDivLX; i += kDivThreads) {
    const int ly = i / kDivLX, lx = i - ly * kDivLX;
    const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    put(i, gy >= 0 && gy < n && gx >= 0 && gx < n, base + (long long)gy * n + gx, gy, gx);
  }
}

// Owned-node walk: node(at, gx, gy, c) for each of the thread's up to 8 nodes that lie in the grid, one column of the
// tile; at: the node's address, c: its index in a halo tile
template <class Node>
__device__ __forceinline__ void div_node_walk(long long base, int n, Node node) {
  const int tid = threadIdx.x;
  const int lx = (tid & 63) + 1, gx = (int)blockIdx.x * kDivTX + (tid & 63);
  const int ly0 = (tid >> 6) * kDivR + 1;
  if (gx >= n) return;
#pragma unroll
  for (int r = 0; r < kDivR; ++r) {
    const int ly = ly0 + r, gy = (int)blockIdx.y * kDivTY + ly - 1;
    if (gy < n) node(base + (long long)gy * n + gx, gx, gy, ly * kDivLX + lx);
  }
}

// the face sum / pair-gradient sum of node (gx, gy), whose halo tiles start at LDS offset c: every ghost face exists on
// the ring, those of the mask's clear bits otherwise
template <bool HARM, Sides S>
__device__ __forceinline__ double node_face_sum(const double* us, const double* ts, int c, int gx, int gy, int n,
                                                int bc) {
  constexpr bool ring = S == Sides::kRing;
  return face_sum_bc<HARM>(us + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n, ring || !(bc & 4),
                           ring || !(bc & 8), ring || !(bc & 1), ring || !(bc & 2));
}

template <bool HARM, Sides S>
__device__ __forceinline__ double node_face_grad_sum(const double* us, const double* ls, const double* ts, int c,
                                                     int gx, int gy, int n, int bc) {
  constexpr bool ring = S == Sides::kRing;
  return face_grad_sum_bc<HARM>(us + c, ls + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n,
                                ring || !(bc & 4), ring || !(bc & 8), ring || !(bc & 1), ring || !(bc & 2));
}

// block b's boundary data (kData; nothing reads it otherwise)
template <Sides S>
__device__ __forceinline__ const double* block_bd(const DivSides& s) {
  return S == Sides::kData ? s.bd + (long long)blockIdx.z * s.bd_stride : nullptr;
}

// y = D_theta u for one tile.  PCG: u = p = z + beta p_old is formed here (header, launch (a)); else g is not read.
// SHIFT: y = D_theta u - sigma * u (the product, then the subtraction, after the face sum's * inv_h2).
// kMask: with the side mask s.bc.  kData (never with PCG): y = A_bd u = D_theta u - sigma * u + b(bd, theta); the
// out-of-grid halo of u holds g beyond Dirichlet sides (bd_halo) and a node on a flux side gains bd_flux_sum * inv_h
// after the face sum's * inv_h2.
template <bool PCG, bool HARM, bool SHIFT, Sides S>
__global__ __launch_bounds__(kDivThreads) void div_apply_kernel(const double* __restrict__ u,
                                                                const double* __restrict__ theta,
                                                                double* __restrict__ y, DivCG g, double inv_h2,
                                                                double sigma, int n, int k, DivSides s) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  __shared__ double red[4];
  constexpr bool BD = S == Sides::kData;
  const int tid = threadIdx.x, b = blockIdx.z, bc = s.bc;
  const double* __restrict__ bd = block_bd<S>(s);
  const long long base = (long long)b * n * n;
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
  div_halo_walk(base, n, [=](int i, bool in, long long at, int gy, int gx) {
    double uv = 0.0, tv = 1.0;
    if (in) {
      uv = u[at];
      tv = theta[at];
      if (PCG && k > 1) uv = uv + beta * pold[at];
    } else if (BD) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ts[i] = tv;
  });
  __syncthreads();

  double acc = 0.0;
  div_node_walk(base, n, [=, &acc](long long at, int gx, int gy, int c) {
    const double uc = us[c];
    double yv = node_face_sum<HARM, S>(us, ts, c, gx, gy, n, bc) * inv_h2;
    if (BD && bd_flux_node(gy, gx, n, bc)) yv = yv + bd_flux_sum(bd, gy, gx, n, bc) * s.inv_h;
    if (SHIFT) yv = yv - sigma * uc;
    y[at] = yv;
    if (PCG) {
      pnew[at] = uc;
      acc = acc + uc * yv;
    }
  });
  if (PCG) {
    const double sum = block_sum(acc, red);
    if (tid == 0) g.ppq[(size_t)b * g.nb + block_id()] = sum;
  }
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
  double acc = 0.0;
  div_node_walk((long long)b * n * n, n, [=, &acc](long long at, int, int, int) {
    g.x[at] = g.x[at] + alpha * p[at];
    const double rv = g.r[at] - alpha * g.q[at];
    g.r[at] = rv;
    acc = acc + rv * rv;
  });
  const double s = block_sum(acc, red);
  if (tid == 0) g.prr[(size_t)b * g.nb + block_id()] = s;
}

// launch (d): partial of r.z; block 0 of a problem settles iteration k (k = 0: the state after init)
__global__ __launch_bounds__(kDivThreads) void div_rz_kernel(DivCG g, int k, double rtol) {
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  double acc = 0.0;
  div_node_walk((long long)b * n * n, n, [=, &acc](long long at, int, int, int) { acc = acc + g.r[at] * g.z[at]; });
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
  double acc = 0.0;
  div_node_walk((long long)b * n * n, n, [=, &acc](long long at, int, int, int) {
    const double fv = f[at];
    g.x[at] = 0.0;
    g.r[at] = fv;
    acc = acc + fv * fv;
  });
  const double s = block_sum(acc, red);
  if (tid == 0) g.prr[(size_t)b * g.nb + block_id()] = s;
}

// warm-started init: x = u0, r = f - D_theta u0 (D_theta u0 as div_apply_kernel forms it, then one subtraction) from
// the halo tiles of u0 and theta; the block's partials of f.f (into the p.q partials, free until iteration 1) and of
// r.r.  The walk and the sums are div_init_kernel's, so for u0 = 0 (D 0 = +0, f - 0 = f) both partials are its bits.
// SHIFT: r = f - (D_theta u0 - sigma * u0), the operator as div_apply_kernel<.., SHIFT> forms it (+0 for u0 = 0 too).
// kMask: with the side mask s.bc.  kData: r = f - A_bd u0 with the halo and the flux term of div_apply_kernel<kData>;
// u0 may be null (zeros: the same operations on 0.0); the first partial is of (f - b)^2, b = A_bd 0 at sigma = 0, i.e.
// b = face_ghost_sum * inv_h2, + bd_flux_sum * inv_h on a flux-side node, then the one subtraction f - b.
template <bool HARM, bool SHIFT, Sides S>
__global__ __launch_bounds__(kDivThreads) void div_init_from_kernel(const double* __restrict__ f,
                                                                    const double* __restrict__ u0,
                                                                    const double* __restrict__ theta, DivCG g,
                                                                    double inv_h2, double sigma, DivSides s) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  __shared__ double red[4];
  constexpr bool BD = S == Sides::kData;
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n, bc = s.bc;
  const double* __restrict__ bd = block_bd<S>(s);
  const long long base = (long long)b * n * n;
  div_halo_walk(base, n, [=](int i, bool in, long long at, int gy, int gx) {
    double uv = 0.0, tv = 1.0;
    if (in) {
      uv = (BD && !u0) ? 0.0 : u0[at];
      tv = theta[at];
    } else if (BD) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ts[i] = tv;
  });
  __syncthreads();

  double accf = 0.0, accr = 0.0;
  div_node_walk(base, n, [=, &accf, &accr](long long at, int gx, int gy, int c) {
    double du = node_face_sum<HARM, S>(us, ts, c, gx, gy, n, bc) * inv_h2;
    double bv = 0.0;
    if (BD) {
      bv = face_ghost_sum(us + c, ts + c, kDivLX, gx > 0, gx + 1 < n, gy > 0, gy + 1 < n, !(bc & 4), !(bc & 8),
                          !(bc & 1), !(bc & 2)) * inv_h2;
      if (bd_flux_node(gy, gx, n, bc)) {
        const double q = bd_flux_sum(bd, gy, gx, n, bc) * s.inv_h;
        du = du + q;
        bv = bv + q;
      }
    }
    if (SHIFT) du = du - sigma * us[c];
    double fv = f[at];
    const double rv = fv - du;
    g.x[at] = us[c];
    g.r[at] = rv;
    if (BD) fv = fv - bv;
    accf = accf + fv * fv;
    accr = accr + rv * rv;
  });
  const double sf = block_sum(accf, red);
  const double sr = block_sum(accr, red);
  if (tid == 0) {
    g.ppq[(size_t)b * g.nb + block_id()] = sf;
    g.prr[(size_t)b * g.nb + block_id()] = sr;
  }
}

// the k = 0 pass after div_init_from_kernel and the sine solve: the block's partial of r.z where iteration 1 reads
// it; |f|^2 from the p.q partials, |r0|^2 from the r.r partials; done at the caller's rtol, so a u0 that already
// satisfies it costs no iteration.  |f| = 0: every block zeroes its tile of x (u = 0 exactly, as the zero start).
__global__ __launch_bounds__(kDivThreads) void div_rz_from_kernel(DivCG g, double rtol) {
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z, n = g.n;
  const long long base = (long long)b * n * n;
  double acc = 0.0;
  div_node_walk(base, n, [=, &acc](long long at, int, int, int) { acc = acc + g.r[at] * g.z[at]; });
  const double s = block_sum(acc, red);
  if (tid == 0) g.prz[0][(size_t)b * g.nb + block_id()] = s;
  const double ff = resum(g.ppq + (size_t)b * g.nb, g.nb, red);
  if (ff == 0.0) div_node_walk(base, n, [=](long long at, int, int, int) { g.x[at] = 0.0; });
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
// order written; f == nullptr is f = 0.  Backward Euler reads no neighbour and stages nothing in LDS, so sides change
// nothing of it: it is instantiated for the ring and the arithmetic mean alone.
// kMask: with the side mask s.bc.  kData: A_bd u at sigma = 0 in place of D_theta u, as div_apply_kernel<kData>.
template <bool CN, bool HARM, Sides S>
__global__ __launch_bounds__(kDivThreads) void div_step_rhs_kernel(const double* __restrict__ u,
                                                                   const double* __restrict__ f,
                                                                   const double* __restrict__ theta,
                                                                   double* __restrict__ rhs, double inv_h2,
                                                                   double sigma, int n, DivSides s) {
  static_assert(CN || (!HARM && S == Sides::kRing), "backward Euler has one instantiation");
  __shared__ double us[CN ? kDivLY * kDivLX : 1];
  __shared__ double ts[CN ? kDivLY * kDivLX : 1];
  constexpr bool BD = S == Sides::kData;
  const int bc = s.bc;
  const double* __restrict__ bd = block_bd<S>(s);
  const long long base = (long long)blockIdx.z * n * n;
  if (CN) {
    div_halo_walk(base, n, [=](int i, bool in, long long at, int gy, int gx) {
      double uv = 0.0, tv = 1.0;
      if (in) {
        uv = u[at];
        tv = theta[at];
      } else if (BD) {
        uv = bd_halo(bd, gy, gx, n, bc);
      }
      us[i] = uv;
      ts[i] = tv;
    });
    __syncthreads();
  }

  div_node_walk(base, n, [=](long long at, int gx, int gy, int c) {
    const double fv = f ? f[at] : 0.0;
    if (CN) {
      double du = node_face_sum<HARM, S>(us, ts, c, gx, gy, n, bc) * inv_h2;
      if (BD && bd_flux_node(gy, gx, n, bc)) du = du + bd_flux_sum(bd, gy, gx, n, bc) * s.inv_h;
      rhs[at] = (2.0 * fv - sigma * us[c]) - du;
    } else {
      rhs[at] = fv - sigma * u[at];
    }
  });
}

// g = scale * G(u, lam; theta), G_a = inv_h2 * sum over a's faces of dc/dtheta_a (u_b - u_a) (lam_b - lam_a): the
// gradient in theta of <lam, D_theta u>.  A gather over the halo tiles of u, lam and theta (3 x 34 x 66 doubles of
// LDS, under the 64 KiB static limit): each node reads its own four faces, nothing is accumulated across nodes.
// kMask: with the side mask s.bc.  kData: u's out-of-grid halo holds g beyond Dirichlet sides, lam's stays 0, so a
// ghost face gives (1 * (g - u_a)) * (0 - lam_a); the prescribed flux does not depend on theta and adds nothing.
template <bool HARM, Sides S>
__global__ __launch_bounds__(kDivThreads) void div_theta_grad_kernel(const double* __restrict__ u,
                                                                     const double* __restrict__ lam,
                                                                     const double* __restrict__ theta,
                                                                     double* __restrict__ gout, double inv_h2,
                                                                     double scale, int n, DivSides s) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ls[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  const int bc = s.bc;
  const double* __restrict__ bd = block_bd<S>(s);
  const long long base = (long long)blockIdx.z * n * n;
  div_halo_walk(base, n, [=](int i, bool in, long long at, int gy, int gx) {
    double uv = 0.0, lv = 0.0, tv = 1.0;
    if (in) {
      uv = u[at];
      lv = lam[at];
      tv = theta[at];
    } else if (S == Sides::kData) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ls[i] = lv;
    ts[i] = tv;
  });
  __syncthreads();

  div_node_walk(base, n, [=](long long at, int gx, int gy, int c) {
    const double gv = node_face_grad_sum<HARM, S>(us, ls, ts, c, gx, gy, n, bc) * inv_h2;
    gout[at] = gv * scale;
  });
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

// ---- Face fluxes theta du/dx, theta du/dy and their wall totals (srpde_div_face_flux, srpde_div_wall_flux and their
// gradients; include/srpde.h states the definitions and the rounding order).  The sides are always a mask with data,
// and a null bd is data of zeros: g = 0 beyond Dirichlet sides, q = 0 through flux sides.

// block b's boundary data, or null
__device__ __forceinline__ const double* flux_bd(const DivSides& s, int b) {
  return s.bd ? s.bd + (long long)b * s.bd_stride : nullptr;
}

// the halo tiles of u (g beyond Dirichlet sides, 0.0 elsewhere outside the grid) and theta (1.0 outside the grid)
__device__ __forceinline__ void flux_stage(const double* __restrict__ u, const double* __restrict__ theta,
                                           const double* __restrict__ bd, double* us, double* ts, long long base, int n,
                                           int bc) {
  div_halo_walk(base, n, [=](int i, bool in, long long at, int gy, int gx) {
    double uv = 0.0, tv = 1.0;
    if (in) {
      uv = u[at];
      tv = theta[at];
    } else if (bd) {
      uv = bd_halo(bd, gy, gx, n, bc);
    }
    us[i] = uv;
    ts[i] = tv;
  });
  __syncthreads();
}

// Fx [B][n][n + 1], Fy [B][n + 1][n].  Every node writes its low-x and its low-y face; the nodes of column n - 1 and
// of row n - 1 write the high wall face too: each face is written once, by one thread.  A face between two nodes is
// (c * (u_hi - u_lo)) * inv_h with c = face_mean(theta_lo, theta_hi); a wall face of a Dirichlet side has c = theta_a
// and the halo's g beyond it; a wall face of a flux side is -q (low wall) or +q (high wall), copied.
template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_face_flux_kernel(const double* __restrict__ u,
                                                                    const double* __restrict__ theta,
                                                                    double* __restrict__ Fx, double* __restrict__ Fy,
                                                                    double inv_h, int n, DivSides s) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  const int b = blockIdx.z, bc = s.bc;
  const double* __restrict__ bd = flux_bd(s, b);
  const long long base = (long long)b * n * n;
  flux_stage(u, theta, bd, us, ts, base, n, bc);

  double* __restrict__ fx = Fx + (long long)b * n * (n + 1);
  double* __restrict__ fy = Fy + (long long)b * (n + 1) * n;
  div_node_walk(base, n, [=](long long, int gx, int gy, int c) {
    const double ua = us[c], ta = ts[c];
    const long long ax = (long long)gy * (n + 1) + gx, ay = (long long)gy * n + gx;
    double w, v;
    if (gx > 0) w = (face_mean<HARM>(ts[c - 1], ta) * (ua - us[c - 1])) * inv_h;
    else if (!(bc & 4)) w = (ta * (ua - us[c - 1])) * inv_h;
    else w = -(bd ? bd[2 * n + gy] : 0.0);
    fx[ax] = w;
    if (gx == n - 1) fx[ax + 1] = !(bc & 8) ? (ta * (us[c + 1] - ua)) * inv_h : (bd ? bd[3 * n + gy] : 0.0);
    if (gy > 0) v = (face_mean<HARM>(ts[c - kDivLX], ta) * (ua - us[c - kDivLX])) * inv_h;
    else if (!(bc & 1)) v = (ta * (ua - us[c - kDivLX])) * inv_h;
    else v = -(bd ? bd[gx] : 0.0);
    fy[ay] = v;
    if (gy == n - 1) fy[ay + n] = !(bc & 2) ? (ta * (us[c + kDivLX] - ua)) * inv_h : (bd ? bd[n + gx] : 0.0);
  });
}

// The adjoint of div_face_flux_kernel in u and theta, a gather: node a collects from its four faces, gW = gFx[i][j],
// gE = gFx[i][j + 1], gN = gFy[i][j], gS = gFy[i + 1][j], with c and d = dc/dtheta_a of face_sum_bc / face_grad_sum_bc
// (theta_a and 1 towards a Dirichlet ghost face, 0 towards a flux side's wall face, whose flux is data):
//     gu_a     = ((cW * gW - cE * gE) + (cN * gN - cS * gS)) * inv_h
//     gtheta_a = (((dW * (u_a - u_W)) * gW + (dE * (u_E - u_a)) * gE)
//               + ((dN * (u_a - u_N)) * gN + (dS * (u_S - u_a)) * gS)) * inv_h
// Either output may be null.  gFx and gFy are read from memory: neighbouring lanes share their faces in the cache.
template <bool HARM>
__global__ __launch_bounds__(kDivThreads) void div_face_flux_grad_kernel(const double* __restrict__ u,
                                                                         const double* __restrict__ theta,
                                                                         const double* __restrict__ gFx,
                                                                         const double* __restrict__ gFy,
                                                                         double* __restrict__ gu,
                                                                         double* __restrict__ gth, double inv_h, int n,
                                                                         DivSides s) {
  __shared__ double us[kDivLY * kDivLX];
  __shared__ double ts[kDivLY * kDivLX];
  const int b = blockIdx.z, bc = s.bc;
  const long long base = (long long)b * n * n;
  flux_stage(u, theta, flux_bd(s, b), us, ts, base, n, bc);

  const double* __restrict__ gx_ = gFx + (long long)b * n * (n + 1);
  const double* __restrict__ gy_ = gFy + (long long)b * (n + 1) * n;
  div_node_walk(base, n, [=](long long at, int gx, int gy, int c) {
    const double ua = us[c], ta = ts[c];
    const long long ax = (long long)gy * (n + 1) + gx, ay = (long long)gy * n + gx;
    const double gW = gx_[ax], gE = gx_[ax + 1], gN = gy_[ay], gS = gy_[ay + n];
    const bool has_w = gx > 0, has_e = gx + 1 < n, has_n = gy > 0, has_s = gy + 1 < n;
    const bool ghost_w = !(bc & 4), ghost_e = !(bc & 8), ghost_n = !(bc & 1), ghost_s = !(bc & 2);
    if (gu) {
      const double cW = has_w ? face_mean<HARM>(ta, ts[c - 1]) : (ghost_w ? ta : 0.0);
      const double cE = has_e ? face_mean<HARM>(ta, ts[c + 1]) : (ghost_e ? ta : 0.0);
      const double cN = has_n ? face_mean<HARM>(ta, ts[c - kDivLX]) : (ghost_n ? ta : 0.0);
      const double cS = has_s ? face_mean<HARM>(ta, ts[c + kDivLX]) : (ghost_s ? ta : 0.0);
      gu[at] = ((cW * gW - cE * gE) + (cN * gN - cS * gS)) * inv_h;
    }
    if (gth) {
      const double dW = has_w ? face_mean_da<HARM>(ta, ts[c - 1]) : (ghost_w ? 1.0 : 0.0);
      const double dE = has_e ? face_mean_da<HARM>(ta, ts[c + 1]) : (ghost_e ? 1.0 : 0.0);
      const double dN = has_n ? face_mean_da<HARM>(ta, ts[c - kDivLX]) : (ghost_n ? 1.0 : 0.0);
      const double dS = has_s ? face_mean_da<HARM>(ta, ts[c + kDivLX]) : (ghost_s ? 1.0 : 0.0);
      gth[at] = (((dW * (ua - us[c - 1])) * gW + (dE * (us[c + 1] - ua)) * gE) +
                 ((dN * (ua - us[c - kDivLX])) * gN + (dS * (us[c + kDivLX] - ua)) * gS)) * inv_h;
    }
  });
}

// the edge node of entry k of a side (the mask's order: row 0, row n - 1, column 0, column n - 1)
__device__ __forceinline__ long long flux_edge_node(int side, int k, int n) {
  const int gy = side == 0 ? 0 : (side == 1 ? n - 1 : k);
  const int gx = side == 2 ? 0 : (side == 3 ? n - 1 : k);
  return (long long)gy * n + gx;
}

// W [B][4] = h * (the sum over a side's n wall faces of the outward flux): (theta_a * (g - u_a)) * inv_h on a Dirichlet
// side -- minus the low wall's face flux, plus the high wall's, the same bits -- and q on a flux side.  grid (4 sides,
// B): thread t adds entries t, t + 256, ... in turn, then block_sum, so the order depends on n alone.
__global__ __launch_bounds__(kRedThreads) void div_wall_flux_kernel(const double* __restrict__ u,
                                                                    const double* __restrict__ theta,
                                                                    double* __restrict__ W, int n, double inv_h,
                                                                    double h, DivSides s) {
  __shared__ double red[4];
  const int side = blockIdx.x, b = blockIdx.y;
  const double* __restrict__ bd = flux_bd(s, b);
  const bool flux = (s.bc >> side) & 1;
  const long long base = (long long)b * n * n;
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += kRedThreads) {
    const double dv = bd ? bd[side * n + k] : 0.0;
    double t = dv;
    if (!flux) {
      const long long at = base + flux_edge_node(side, k, n);
      t = (theta[at] * (dv - u[at])) * inv_h;
    }
    acc = acc + t;
  }
  const double sum = block_sum(acc, red);
  if (threadIdx.x == 0) W[(long long)b * 4 + side] = h * sum;
}

// The adjoint of div_wall_flux_kernel, three [B][4][n] outputs (any may be null), with w = gW[b][side] * h and a the
// edge node of entry k:  Dirichlet side: gu_edge = -((theta_a * inv_h) * w), gtheta_edge = ((g - u_a) * inv_h) * w,
// gbd = (theta_a * inv_h) * w;  flux side: 0.0, 0.0 and w.  grid (ceil(n / 256), 4, B), as div_bd_grad_kernel.
__global__ __launch_bounds__(256) void div_wall_flux_grad_kernel(const double* __restrict__ gW,
                                                                 const double* __restrict__ u,
                                                                 const double* __restrict__ theta,
                                                                 double* __restrict__ gu_edge,
                                                                 double* __restrict__ gth_edge,
                                                                 double* __restrict__ gbd, int n, double inv_h,
                                                                 double h, DivSides s) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x, side = blockIdx.y, b = blockIdx.z;
  if (k >= n) return;
  const double* __restrict__ bd = flux_bd(s, b);
  const double w = gW[(long long)b * 4 + side] * h;
  const long long o = ((long long)b * 4 + side) * n + k;
  double guv = 0.0, gtv = 0.0, gbv = w;
  if (!((s.bc >> side) & 1)) {
    const long long at = (long long)b * n * n + flux_edge_node(side, k, n);
    const double dv = bd ? bd[side * n + k] : 0.0;
    const double tw = theta[at] * inv_h;
    guv = -(tw * w);
    gtv = ((dv - u[at]) * inv_h) * w;
    gbv = tw * w;
  }
  if (gu_edge) gu_edge[o] = guv;
  if (gth_edge) gth_edge[o] = gtv;
  if (gbd) gbd[o] = gbv;
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

// The one place where run-time flags become template arguments: launch(SHIFT, HARM, SIDES, EXTRA) is called with the
// std::integral_constant of each (extra: PCG of the apply kernel, CN of the step's).  A launcher's callable holds its
// one launch statement and names no instantiation that nobody launches (PCG with data, backward Euler with sides).
template <class Launch>
void div_dispatch(const DivSides& s, bool shift, bool harm, bool extra, Launch launch) {
  auto flag = [](bool v, auto fn) { v ? fn(std::true_type{}) : fn(std::false_type{}); };
  flag(shift, [&](auto SHIFT) {
    flag(harm, [&](auto HARM) {
      flag(extra, [&](auto EXTRA) {
        if (s.kind == Sides::kRing) launch(SHIFT, HARM, std::integral_constant<Sides, Sides::kRing>{}, EXTRA);
        if (s.kind == Sides::kMask) launch(SHIFT, HARM, std::integral_constant<Sides, Sides::kMask>{}, EXTRA);
        if (s.kind == Sides::kData) launch(SHIFT, HARM, std::integral_constant<Sides, Sides::kData>{}, EXTRA);
      });
    });
  });
}

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

static int div_check_ws(const char* name, int B, int n, const void* ws, size_t ws_bytes, const DivSides& s) {
  if (!ws) SRPDE_FAIL(kErrArg, "%s: null workspace", name);
  if (!aligned16(ws)) SRPDE_FAIL(kErrAlign, "%s: workspace not 16-byte aligned", name);
  const size_t need = carve(nullptr, B, n, s).bytes;
  if (ws_bytes < need) SRPDE_FAIL(kErrWorkspace, "%s: workspace too small (%zu bytes, needs %zu)", name, ws_bytes, need);
  return 0;
}

// the sine-transform plan for n, or the separable plan for n and the side mask
static int div_check_plan(const char* name, int n, const void* plan, size_t plan_bytes, const DivSides& s) {
  if (!plan) SRPDE_FAIL(kErrArg, "%s: null plan", name);
  if (reinterpret_cast<uintptr_t>(plan) & 7u) SRPDE_FAIL(kErrAlign, "%s: plan not 8-byte aligned", name);
  if (separable(s)) {
    if (plan_bytes != sep_plan_bytes_for(n, s.bc))
      SRPDE_FAIL(kErrWorkspace, "%s: a plan of %zu bytes is not a plan for n=%d and bc=%d (srpde_poisson_sep_plan_size: %zu)",
                 name, plan_bytes, n, s.bc, sep_plan_bytes_for(n, s.bc));
    return 0;
  }
  if (plan_bytes != dst_plan_bytes_for(n))
    SRPDE_FAIL(kErrWorkspace, "%s: a plan of %zu bytes is not a plan for n=%d (srpde_poisson_dst_plan_size: %zu)", name,
               plan_bytes, n, dst_plan_bytes_for(n));
  return 0;
}

// the side mask of a *_bc or *_bd entry, then the data of a *_bd entry; the ring has neither
static int div_check_sides(const char* name, int n, const DivSides& s) {
  if (s.kind == Sides::kRing) return 0;
  if (s.bc < 0 || s.bc > 15)
    SRPDE_FAIL(kErrArg, "%s: bc=%d is not a side mask (bits 0..3: row 0, row n-1, column 0, column n-1; set = zero flux)",
               name, s.bc);
  if (s.kind == Sides::kMask) return 0;
  if (!s.bd) SRPDE_FAIL(kErrArg, "%s: null boundary data", name);
  if (reinterpret_cast<uintptr_t>(s.bd) & 7u) SRPDE_FAIL(kErrAlign, "%s: bd not 8-byte aligned", name);
  if (s.bd_stride != 0 && s.bd_stride != 4LL * n)
    SRPDE_FAIL(kErrArg, "%s: bd_stride=%lld is neither 4 n = %lld ([B][4][n]) nor 0 (one [4][n] for every problem)", name,
               s.bd_stride, 4LL * n);
  return 0;
}

// all four sides zero-flux is singular without a shift
static int div_check_singular(const char* name, const DivSides& s, const char* what, double sigma) {
  if (s.bc == 15 && sigma == 0.0)
    SRPDE_FAIL(kErrArg, "%s: four zero-flux sides (bc=15) with %s=0 is singular (the constants): it needs a shift > 0",
               name, what);
  return 0;
}

// sigma >= 0 and finite; the message names the entry
static int div_check_sigma(const char* name, const char* what, double sigma) {
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) SRPDE_FAIL(kErrArg, "%s: %s=%g must be >= 0 and finite", name, what, sigma);
  return 0;
}

static int div_check_inv_h2(const char* name, double inv_h2) {
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  return 0;
}

static int div_check_rtol(const char* name, double rtol) {
  if (!(rtol >= 0.0)) SRPDE_FAIL(kErrArg, "%s: rtol=%g must be >= 0", name, rtol);
  return 0;
}

static int div_check_aligned8(const char* name, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  if (bits & 7u) SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  return 0;
}

// out (named what in the message) is none of the inputs; a null input is one the entry does not have
static int div_check_alias(const char* name, const char* what, const void* out, std::initializer_list<const void*> in) {
  for (const void* p : in)
    if (out == p) SRPDE_FAIL(kErrArg, "%s: %s aliases an input (a node reads its neighbours)", name, what);
  return 0;
}

// step (c): z = M^-1 r -- the sine-transform solve, or the separable solve with the side mask its plan was built for
static int div_precondition(const char* name, const DivCG& g, int B, int n, const DivSides& s, const void* plan,
                            hipStream_t stream, double sigma_p) {
  if (!separable(s)) return dst_solve_launch(name, g.r, nullptr, g.z, B, n, plan, g.dst_ws, stream, sigma_p);
  return sep_solve_launch(name, g.r, g.z, B, n, plan, g.sep_ws, stream, sigma_p);
}

// launch (a) (pcg: u = g.z, y = g.q), or the operator alone (g is not read); sigma = 0 is the unshifted kernel
static void div_apply_run(bool pcg, const double* u, const double* theta, double* y, const DivCG& g, int B, int n,
                          int face_mean, double inv_h2, double sigma, int k, const DivSides& s, hipStream_t stream) {
  div_dispatch(s, sigma != 0.0, face_mean != 0, pcg, [&](auto SHIFT, auto HARM, auto SIDES, auto PCG) {
    if constexpr (!(PCG() && SIDES() == Sides::kData))   // the iteration has no data: b went into f
      hipLaunchKernelGGL((div_apply_kernel<PCG(), HARM(), SHIFT(), SIDES()>), div_grid(B, n), dim3(kDivThreads), 0,
                         stream, u, theta, y, g, inv_h2, SHIFT() ? sigma : 0.0, n, k, s);
  });
}

extern "C" {

size_t srpde_div_cg_workspace_size_bc(int B, int n) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN) return 0;
  return carve(nullptr, B, n, mask_sides(0)).bytes;
}

size_t srpde_div_cg_workspace_size(int B, int n) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN) return 0;
  return carve(nullptr, B, n, ring_sides()).bytes;
}

size_t srpde_div_cg_done_offset(int B, int n) {
  if (B <= 0 || B > kDivMaxB || n < 2 || n > kDivMaxN) return 0;
  return (size_t)(reinterpret_cast<char*>(carve(nullptr, B, n, ring_sides()).done) - static_cast<char*>(nullptr));
}

// srpde_div_apply, srpde_div_apply_shift, srpde_div_apply_bc and srpde_div_apply_bd
static int div_apply_launch(const char* name, const double* u, const double* theta, double* y, int B, int n,
                            int face_mean, double inv_h2, double sigma, const DivSides& s, hipStream_t stream) {
  SRPDE_CHECK_ARG(u && theta && y, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sides(name, n, s)) return rc;
  if (int rc = div_check_inv_h2(name, inv_h2)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_aligned8(name, {u, theta, y})) return rc;
  if (int rc = div_check_alias(name, "y", y, {u, theta, s.bd})) return rc;
  div_apply_run(false, u, theta, y, DivCG{}, B, n, face_mean, inv_h2, sigma, 0, s, stream);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_apply(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                    hipStream_t stream) {
  return div_apply_launch("srpde_div_apply", u, theta, y, B, n, face_mean, inv_h2, 0.0, ring_sides(), stream);
}

int srpde_div_apply_shift(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                          double sigma, hipStream_t stream) {
  return div_apply_launch("srpde_div_apply_shift", u, theta, y, B, n, face_mean, inv_h2, sigma, ring_sides(), stream);
}

int srpde_div_apply_bc(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                       double sigma, int bc, hipStream_t stream) {
  return div_apply_launch("srpde_div_apply_bc", u, theta, y, B, n, face_mean, inv_h2, sigma, mask_sides(bc), stream);
}

int srpde_div_apply_bd(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                       double sigma, int bc, const double* bd, long long bd_stride, hipStream_t stream) {
  return div_apply_launch("srpde_div_apply_bd", u, theta, y, B, n, face_mean, inv_h2, sigma,
                          data_sides(bc, bd, bd_stride, std::sqrt(inv_h2)), stream);
}

// srpde_div_step_rhs, srpde_div_step_rhs_bc and srpde_div_step_rhs_bd
static int div_step_rhs(const char* name, const double* u, const double* f, const double* theta, double* rhs, int B,
                        int n, int face_mean, double sigma, int cn, const DivSides& s, hipStream_t stream) {
  SRPDE_CHECK_ARG(u && theta && rhs, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sides(name, n, s)) return rc;
  if (cn != 0 && cn != 1) SRPDE_FAIL(kErrArg, "%s: cn=%d (0 backward Euler, 1 Crank-Nicolson)", name, cn);
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_aligned8(name, {u, f, theta, rhs})) return rc;
  if (int rc = div_check_alias(name, "rhs", rhs, {u, theta, f, s.bd})) return rc;
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  div_dispatch(s, false, face_mean != 0, cn != 0, [&](auto, auto HARM, auto SIDES, auto CN) {
    // backward Euler reads no neighbour: whatever the mean and the sides, its one kernel
    hipLaunchKernelGGL((div_step_rhs_kernel<CN(), CN() && HARM(), CN() ? SIDES() : Sides::kRing>), div_grid(B, n),
                       dim3(kDivThreads), 0, stream, u, f, theta, rhs, inv_h2, sigma, n, s);
  });
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_step_rhs(const double* u, const double* f, const double* theta, double* rhs, int B, int n, int face_mean,
                       double sigma, int cn, hipStream_t stream) {
  return div_step_rhs("srpde_div_step_rhs", u, f, theta, rhs, B, n, face_mean, sigma, cn, ring_sides(), stream);
}

int srpde_div_step_rhs_bc(const double* u, const double* f, const double* theta, double* rhs, int B, int n,
                          int face_mean, double sigma, int cn, int bc, hipStream_t stream) {
  return div_step_rhs("srpde_div_step_rhs_bc", u, f, theta, rhs, B, n, face_mean, sigma, cn, mask_sides(bc), stream);
}

int srpde_div_step_rhs_bd(const double* u, const double* f, const double* theta, double* rhs, int B, int n,
                          int face_mean, double sigma, int cn, int bc, const double* bd, long long bd_stride,
                          hipStream_t stream) {
  const char* name = "srpde_div_step_rhs_bd";
  const DivSides s = data_sides(bc, bd, bd_stride, (double)(n - 1));
  if (int rc = div_check_sides(name, n, s)) return rc;
  // backward Euler reads no neighbour, so no data either: srpde_div_step_rhs_bc's checks and launch
  return div_step_rhs(name, u, f, theta, rhs, B, n, face_mean, sigma, cn, cn == 1 ? s : mask_sides(bc), stream);
}

// srpde_div_cg_init, srpde_div_cg_init_shift and srpde_div_cg_init_bc (the zero start has r = f whatever sigma is: only
// M changes)
static int div_cg_init(const char* name, const double* f, int B, int n, double sigma_p, const void* plan,
                       size_t plan_bytes, void* ws, size_t ws_bytes, const DivSides& s, hipStream_t stream) {
  SRPDE_CHECK_ARG(f, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, 0)) return rc;
  if (int rc = div_check_sides(name, n, s)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, s, "sigma_p", sigma_p)) return rc;
  if (reinterpret_cast<uintptr_t>(f) & 7u) SRPDE_FAIL(kErrAlign, "%s: f not 8-byte aligned", name);
  if (int rc = div_check_plan(name, n, plan, plan_bytes, s)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, s)) return rc;
  DivCG g = carve(ws, B, n, s);
  hipLaunchKernelGGL(div_init_kernel, div_grid(B, n), dim3(kDivThreads), 0, stream, f, g);
  SRPDE_LAUNCH_CHECK(name);
  if (int rc = div_precondition(name, g, B, n, s, plan, stream, sigma_p)) return rc;
  // rtol 0: only |f| = 0 is done before the first iteration
  hipLaunchKernelGGL(div_rz_kernel, div_grid(B, n), dim3(kDivThreads), 0, stream, g, 0, 0.0);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_cg_init(const double* f, int B, int n, const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                      hipStream_t stream) {
  return div_cg_init("srpde_div_cg_init", f, B, n, 0.0, plan, plan_bytes, ws, ws_bytes, ring_sides(), stream);
}

int srpde_div_cg_init_shift(const double* f, int B, int n, double sigma_p, const void* plan, size_t plan_bytes,
                            void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init("srpde_div_cg_init_shift", f, B, n, sigma_p, plan, plan_bytes, ws, ws_bytes, ring_sides(), stream);
}

int srpde_div_cg_init_bc(const double* f, int B, int n, int bc, double sigma_p, const void* plan, size_t plan_bytes,
                         void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init("srpde_div_cg_init_bc", f, B, n, sigma_p, plan, plan_bytes, ws, ws_bytes, mask_sides(bc), stream);
}

// srpde_div_cg_init_from, its _shift and _bc, and srpde_div_cg_init_from_bd (u0 may be null there: zeros)
static int div_cg_init_from(const char* name, const double* f, const double* u0, const double* theta, int B, int n,
                            int face_mean, double sigma, double sigma_p, double rtol, const void* plan,
                            size_t plan_bytes, void* ws, size_t ws_bytes, const DivSides& s, hipStream_t stream) {
  SRPDE_CHECK_ARG(f && (u0 || s.kind == Sides::kData) && theta, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sides(name, n, s)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, s, "sigma", sigma)) return rc;
  if (int rc = div_check_singular(name, s, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_aligned8(name, {f, u0, theta})) return rc;
  if (int rc = div_check_rtol(name, rtol)) return rc;
  if (int rc = div_check_plan(name, n, plan, plan_bytes, s)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, s)) return rc;
  DivCG g = carve(ws, B, n, s);
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  div_dispatch(s, sigma != 0.0, face_mean != 0, false, [&](auto SHIFT, auto HARM, auto SIDES, auto) {
    hipLaunchKernelGGL((div_init_from_kernel<HARM(), SHIFT(), SIDES()>), grid, block, 0, stream, f, u0, theta, g,
                       inv_h2, SHIFT() ? sigma : 0.0, s);
  });
  SRPDE_LAUNCH_CHECK(name);
  if (int rc = div_precondition(name, g, B, n, s, plan, stream, sigma_p)) return rc;
  hipLaunchKernelGGL(div_rz_from_kernel, grid, block, 0, stream, g, rtol);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_cg_init_from(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                           double rtol, const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                           hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from", f, u0, theta, B, n, face_mean, 0.0, 0.0, rtol, plan, plan_bytes,
                          ws, ws_bytes, ring_sides(), stream);
}

int srpde_div_cg_init_from_shift(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                                 double sigma, double sigma_p, double rtol, const void* plan, size_t plan_bytes,
                                 void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from_shift", f, u0, theta, B, n, face_mean, sigma, sigma_p, rtol, plan,
                          plan_bytes, ws, ws_bytes, ring_sides(), stream);
}

int srpde_div_cg_init_from_bc(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                              int bc, double sigma, double sigma_p, double rtol, const void* plan, size_t plan_bytes,
                              void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from_bc", f, u0, theta, B, n, face_mean, sigma, sigma_p, rtol, plan,
                          plan_bytes, ws, ws_bytes, mask_sides(bc), stream);
}

int srpde_div_cg_init_from_bd(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                              int bc, double sigma, double sigma_p, double rtol, const double* bd, long long bd_stride,
                              const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_init_from("srpde_div_cg_init_from_bd", f, u0, theta, B, n, face_mean, sigma, sigma_p, rtol, plan,
                          plan_bytes, ws, ws_bytes, data_sides(bc, bd, bd_stride, (double)(n - 1)), stream);
}

// srpde_div_theta_grad, srpde_div_theta_grad_bc and srpde_div_theta_grad_bd
static int div_theta_grad(const char* name, const double* u, const double* lam, const double* theta, double* g_out,
                          int B, int n, int face_mean, double inv_h2, double scale, const DivSides& s,
                          hipStream_t stream) {
  SRPDE_CHECK_ARG(u && lam && theta && g_out, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sides(name, n, s)) return rc;
  if (int rc = div_check_inv_h2(name, inv_h2)) return rc;
  if (!std::isfinite(scale)) SRPDE_FAIL(kErrArg, "%s: scale=%g must be finite", name, scale);
  if (int rc = div_check_aligned8(name, {u, lam, theta, g_out})) return rc;
  if (int rc = div_check_alias(name, "g_out", g_out, {u, lam, theta, s.bd})) return rc;
  div_dispatch(s, false, face_mean != 0, false, [&](auto, auto HARM, auto SIDES, auto) {
    hipLaunchKernelGGL((div_theta_grad_kernel<HARM(), SIDES()>), div_grid(B, n), dim3(kDivThreads), 0, stream, u, lam,
                       theta, g_out, inv_h2, scale, n, s);
  });
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_theta_grad(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                         int face_mean, double inv_h2, double scale, hipStream_t stream) {
  return div_theta_grad("srpde_div_theta_grad", u, lam, theta, g_out, B, n, face_mean, inv_h2, scale, ring_sides(),
                        stream);
}

int srpde_div_theta_grad_bc(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                            int face_mean, double inv_h2, double scale, int bc, hipStream_t stream) {
  return div_theta_grad("srpde_div_theta_grad_bc", u, lam, theta, g_out, B, n, face_mean, inv_h2, scale,
                        mask_sides(bc), stream);
}

int srpde_div_theta_grad_bd(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                            int face_mean, double inv_h2, double scale, int bc, const double* bd, long long bd_stride,
                            hipStream_t stream) {
  return div_theta_grad("srpde_div_theta_grad_bd", u, lam, theta, g_out, B, n, face_mean, inv_h2, scale,
                        data_sides(bc, bd, bd_stride, 0.0), stream);
}

// srpde_div_cg_iterate, its _shift and its _bc (a solve with data iterates without it: one of these)
static int div_cg_iterate(const char* name, const double* theta, int B, int n, int face_mean, double sigma,
                          double sigma_p, double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes,
                          void* ws, size_t ws_bytes, const DivSides& s, hipStream_t stream) {
  SRPDE_CHECK_ARG(theta, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sides(name, n, s)) return rc;
  if (int rc = div_check_sigma(name, "sigma", sigma)) return rc;
  if (int rc = div_check_sigma(name, "sigma_p", sigma_p)) return rc;
  if (int rc = div_check_singular(name, s, "sigma", sigma)) return rc;
  if (int rc = div_check_singular(name, s, "sigma_p", sigma_p)) return rc;
  if (reinterpret_cast<uintptr_t>(theta) & 7u) SRPDE_FAIL(kErrAlign, "%s: theta not 8-byte aligned", name);
  if (int rc = div_check_rtol(name, rtol)) return rc;
  if (k_begin < 1 || k_count < 0 || k_count > INT32_MAX - k_begin)
    SRPDE_FAIL(kErrArg, "%s: k_begin=%d k_count=%d (iterations count from 1)", name, k_begin, k_count);
  if (int rc = div_check_plan(name, n, plan, plan_bytes, s)) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, s)) return rc;
  DivCG g = carve(ws, B, n, s);
  const double inv_h2 = (double)(n - 1) * (double)(n - 1);
  const dim3 grid = div_grid(B, n), block(kDivThreads);
  for (int k = k_begin; k < k_begin + k_count; ++k) {
    div_apply_run(true, g.z, theta, g.q, g, B, n, face_mean, inv_h2, sigma, k, s, stream);
    hipLaunchKernelGGL(div_update_kernel, grid, block, 0, stream, g, k);
    SRPDE_LAUNCH_CHECK(name);
    if (int rc = div_precondition(name, g, B, n, s, plan, stream, sigma_p)) return rc;
    hipLaunchKernelGGL(div_rz_kernel, grid, block, 0, stream, g, k, rtol);
    SRPDE_LAUNCH_CHECK(name);
  }
  return 0;
}

int srpde_div_cg_iterate(const double* theta, int B, int n, int face_mean, double rtol, int k_begin, int k_count,
                         const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  return div_cg_iterate("srpde_div_cg_iterate", theta, B, n, face_mean, 0.0, 0.0, rtol, k_begin, k_count, plan,
                        plan_bytes, ws, ws_bytes, ring_sides(), stream);
}

int srpde_div_cg_iterate_shift(const double* theta, int B, int n, int face_mean, double sigma, double sigma_p,
                               double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes, void* ws,
                               size_t ws_bytes, hipStream_t stream) {
  return div_cg_iterate("srpde_div_cg_iterate_shift", theta, B, n, face_mean, sigma, sigma_p, rtol, k_begin, k_count,
                        plan, plan_bytes, ws, ws_bytes, ring_sides(), stream);
}

int srpde_div_cg_iterate_bc(const double* theta, int B, int n, int face_mean, int bc, double sigma, double sigma_p,
                            double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes, void* ws,
                            size_t ws_bytes, hipStream_t stream) {
  return div_cg_iterate("srpde_div_cg_iterate_bc", theta, B, n, face_mean, sigma, sigma_p, rtol, k_begin, k_count,
                        plan, plan_bytes, ws, ws_bytes, mask_sides(bc), stream);
}

int srpde_div_bd_grad(const double* lam, const double* theta, double* out, int B, int n, double inv_h2, int bc,
                      hipStream_t stream) {
  const char* name = "srpde_div_bd_grad";
  SRPDE_CHECK_ARG(lam && theta && out, "%s: null pointer", name);
  if (int rc = div_check(name, B, n, 0)) return rc;
  if (int rc = div_check_sides(name, n, mask_sides(bc))) return rc;
  if (int rc = div_check_inv_h2(name, inv_h2)) return rc;
  if (int rc = div_check_aligned8(name, {lam, theta, out})) return rc;
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
  if (int rc = div_check_aligned8(name, {u, resid})) return rc;
  if (int rc = div_check_ws(name, B, n, ws, ws_bytes, ring_sides())) return rc;
  DivCG g = carve(ws, B, n, ring_sides());
  const long long total = (long long)B * n * n;
  hipLaunchKernelGGL(div_finish_kernel, dim3(elementwise_grid(total)), dim3(256), 0, stream, g, u, iters, resid, total,
                     B);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

// the checks the four flux entries share: the operator's shape limits, the face mean, the mask, inv_h2, and the data,
// which may be null here (zeros)
static int div_flux_check(const char* name, int B, int n, int face_mean, double inv_h2, int bc, const double* bd,
                          long long bd_stride) {
  if (int rc = div_check(name, B, n, face_mean)) return rc;
  if (int rc = div_check_sides(name, n, mask_sides(bc))) return rc;
  if (int rc = div_check_inv_h2(name, inv_h2)) return rc;
  if (reinterpret_cast<uintptr_t>(bd) & 7u) SRPDE_FAIL(kErrAlign, "%s: bd not 8-byte aligned", name);
  if (bd_stride != 0 && bd_stride != 4LL * n)
    SRPDE_FAIL(kErrArg, "%s: bd_stride=%lld is neither 4 n = %lld ([B][4][n]) nor 0 (one [4][n] for every problem)", name,
               bd_stride, 4LL * n);
  return 0;
}

int srpde_div_face_flux(const double* u, const double* theta, double* Fx, double* Fy, int B, int n, int face_mean,
                        double inv_h2, int bc, const double* bd, long long bd_stride, hipStream_t stream) {
  const char* name = "srpde_div_face_flux";
  SRPDE_CHECK_ARG(u && theta && Fx && Fy, "%s: null pointer", name);
  if (int rc = div_flux_check(name, B, n, face_mean, inv_h2, bc, bd, bd_stride)) return rc;
  if (int rc = div_check_aligned8(name, {u, theta, Fx, Fy})) return rc;
  if (int rc = div_check_alias(name, "Fx", Fx, {u, theta, bd, Fy})) return rc;
  if (int rc = div_check_alias(name, "Fy", Fy, {u, theta, bd})) return rc;
  const DivSides s = data_sides(bc, bd, bd_stride, std::sqrt(inv_h2));
  div_dispatch(s, false, face_mean != 0, false, [&](auto, auto HARM, auto, auto) {
    hipLaunchKernelGGL((div_face_flux_kernel<HARM()>), div_grid(B, n), dim3(kDivThreads), 0, stream, u, theta, Fx, Fy,
                       s.inv_h, n, s);
  });
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_face_flux_grad(const double* u, const double* theta, const double* gFx, const double* gFy, double* gu,
                             double* gtheta, int B, int n, int face_mean, double inv_h2, int bc, const double* bd,
                             long long bd_stride, hipStream_t stream) {
  const char* name = "srpde_div_face_flux_grad";
  SRPDE_CHECK_ARG(u && theta && gFx && gFy, "%s: null pointer", name);
  if (int rc = div_flux_check(name, B, n, face_mean, inv_h2, bc, bd, bd_stride)) return rc;
  if (int rc = div_check_aligned8(name, {u, theta, gFx, gFy, gu, gtheta})) return rc;
  if (gu)
    if (int rc = div_check_alias(name, "gu", gu, {u, theta, gFx, gFy, bd, gtheta})) return rc;
  if (gtheta)
    if (int rc = div_check_alias(name, "gtheta", gtheta, {u, theta, gFx, gFy, bd})) return rc;
  if (!gu && !gtheta) return 0;
  const DivSides s = data_sides(bc, bd, bd_stride, std::sqrt(inv_h2));
  div_dispatch(s, false, face_mean != 0, false, [&](auto, auto HARM, auto, auto) {
    hipLaunchKernelGGL((div_face_flux_grad_kernel<HARM()>), div_grid(B, n), dim3(kDivThreads), 0, stream, u, theta,
                       gFx, gFy, gu, gtheta, s.inv_h, n, s);
  });
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_wall_flux(const double* u, const double* theta, double* W, int B, int n, int face_mean, double inv_h2,
                        int bc, const double* bd, long long bd_stride, hipStream_t stream) {
  const char* name = "srpde_div_wall_flux";
  SRPDE_CHECK_ARG(u && theta && W, "%s: null pointer", name);
  if (int rc = div_flux_check(name, B, n, face_mean, inv_h2, bc, bd, bd_stride)) return rc;
  if (int rc = div_check_aligned8(name, {u, theta, W})) return rc;
  if (int rc = div_check_alias(name, "W", W, {u, theta, bd})) return rc;
  const DivSides s = data_sides(bc, bd, bd_stride, std::sqrt(inv_h2));
  hipLaunchKernelGGL(div_wall_flux_kernel, dim3(4, B), dim3(kRedThreads), 0, stream, u, theta, W, n, s.inv_h,
                     1.0 / s.inv_h, s);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

int srpde_div_wall_flux_grad(const double* gW, const double* u, const double* theta, double* gu_edge,
                             double* gtheta_edge, double* gbd, int B, int n, double inv_h2, int bc, const double* bd,
                             long long bd_stride, hipStream_t stream) {
  const char* name = "srpde_div_wall_flux_grad";
  SRPDE_CHECK_ARG(gW && u && theta, "%s: null pointer", name);
  if (int rc = div_flux_check(name, B, n, 0, inv_h2, bc, bd, bd_stride)) return rc;
  if (int rc = div_check_aligned8(name, {gW, u, theta, gu_edge, gtheta_edge, gbd})) return rc;
  for (double* out : {gu_edge, gtheta_edge, gbd})
    if (out)
      if (int rc = div_check_alias(name, "an output", out, {gW, u, theta, bd})) return rc;
  if ((gu_edge && (gu_edge == gtheta_edge || gu_edge == gbd)) || (gbd && gbd == gtheta_edge))
    SRPDE_FAIL(kErrArg, "%s: two outputs are the same buffer", name);
  if (!gu_edge && !gtheta_edge && !gbd) return 0;
  const DivSides s = data_sides(bc, bd, bd_stride, std::sqrt(inv_h2));
  hipLaunchKernelGGL(div_wall_flux_grad_kernel, dim3(ceil_div(n, 256), 4, B), dim3(256), 0, stream, gW, u, theta,
                     gu_edge, gtheta_edge, gbd, n, s.inv_h, 1.0 / s.inv_h, s);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

}  // extern "C"
