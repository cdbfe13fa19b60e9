// Weighted-Jacobi sweeps on an n x n grid, fp64, gfx950: the post-smoother of the cascade.  One kernel,
// relax_kernel<Op>, for two operators (a zero ghost ring outside the grid; E is x + 1, S is y + 1; c = 0.25 * omega,
// formed on the host):
//
//                    PointwiseOp:  theta * L u = f                      DivOp<HARM>:  div(theta grad u) = f
//     once per node  g  = f / (theta * inv_h2)                          g = f / inv_h2
//                                                                       w = omega / ((cE + cW) + (cS + cN))
//     per sweep      s  = (uN + uS) + (uW + uE)                         a  = (cE*(uE - u) + cW*(uW - u)) +
//                    r  = (s - 4.0 * u) - g                                  (cS*(uS - u) + cN*(uN - u))
//                    u' = u + c * r                                     u' = u + w * (a - g)
//
// Every operation is rounded once in this order (contraction is off for the whole file).  The divergence operator is
// that of srpde_div_apply, its face coefficients those of div_stencil.h (HARM: face_mean 1).  Jacobi: every u' comes
// from the previous sweep's u.  The error operators are I + (omega / 4) A, symmetric with eigenvalues
// 1 - omega (sin^2(a / 2) + sin^2(b / 2)), and I - omega diag(-D_theta)^-1 (-D_theta), where -D_theta is a symmetric,
// weakly diagonally dominant M-matrix with its Jacobi spectrum in [0, 2]: for 0 < omega <= 1 nothing grows.
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
// eight u values and the operator's sweep-invariant data live in registers for the whole launch, so a sweep reads from
// LDS only the left and right neighbours and the two rows above and below the wave's strip, and writes its new values
// for the neighbours.  LDS: 2 planes x 64 x 64 x 8 B = 64 KiB.  A row of 64 doubles covers the 64 4-byte banks twice
// over in one 32-lane group each: no bank conflicts.  Per thread, beside u[8]:
//     PointwiseOp   g[8]                16 doubles with u: two workgroups (16 waves) per CU
//     DivOp         g[8], w[8]          formed once per launch while staging -- theta goes through the LDS plane that
//                   cE[8]               sweep 1 overwrites -- so the harmonic mean's divisions are paid once per launch
//                   cW[8]               = cE of lane x - 1, fetched once per launch with a wave shuffle (a wave is one
//                                         patch row); the means are commutative, so the bits are the same
//                   cV[9]               cV[r] is the face between rows r - 1 and r: cN of row r and cS of row r - 1
//                                       49 doubles with u = 98 VGPRs
// A face with exactly one end inside the grid carries theta of that end (the ghost-face rule of the in-grid node; the
// outside node is fixed at 0 and never reads it), a face with no end inside carries 1.  DivOp<HARM, true>
// (srpde_div_relax_bc): 0.0 instead of theta of that end when the outside end lies beyond a zero-flux side.
//
// srpde_div_relax_bd (relax_tile<DivOp<HARM, true>, true>): the positions straight beyond a Dirichlet side's edge nodes
// hold the boundary value g instead of 0 (fixed, like every position outside the grid) and a node on a flux side forms
// g = (f - ((qE + qW) + (qS + qN)) * inv_h) / inv_h2; both once per launch, the sweep is the same code.
//
// Every u' is a pure function of its five u values and the node's constants in a fixed order, so the result does not
// depend on T, K or how the sweeps are split over launches: it is bit-equal to one plain pass per sweep.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)
#include "div_stencil.h"                               // after the pragma: its functions take the mode of this file

namespace srpde {
namespace {

constexpr int kRelaxT = 48;                            // output tile
constexpr int kRelaxK = 8;                             // sweeps per launch = halo width
constexpr int kRelaxP = kRelaxT + 2 * kRelaxK;         // patch side
constexpr int kRelaxWaves = 8;
constexpr int kRelaxThreads = 64 * kRelaxWaves;
constexpr int kRelaxR = kRelaxP / kRelaxWaves;         // rows per thread
static_assert(kRelaxP == 64, "one patch column per lane");
static_assert(kRelaxR * kRelaxWaves == kRelaxP && kRelaxR <= 32, "the waves' strips tile the patch");
constexpr int kRelaxMaxN = 16384;

// What an operator keeps per thread between sweeps and its update of one node.  wt is the kernel's weight argument.
struct PointwiseOp {
  static constexpr bool kFaces = false;
  double c, g[kRelaxR];
  __device__ __forceinline__ explicit PointwiseOp(double wt) : c(wt) {}
  static __device__ __forceinline__ double rhs(double f, double theta, double inv_h2) { return f / (theta * inv_h2); }
  __device__ __forceinline__ double update(int r, double cur, double prev, double dn, double uW, double uE) const {
    const double sum = (prev + dn) + (uW + uE);
    const double res = (sum - 4.0 * cur) - g[r];
    return cur + c * res;
  }
};

// BC: with the side mask bc of srpde_div_relax_bc (bit 0 the row 0 side, 1 row n - 1, 2 column 0, 3 column n - 1; set:
// zero flux).  Only form() differs: a face with one end inside the grid carries 0.0 instead of theta of that end when
// that side is zero-flux -- face_sum_bc's coefficient -- so the sweep multiplies the zero in (0 * (0 - u) = -+0) and
// keeps face_sum_bc's order.  The mask is a kernel argument (uniform, scalar registers) read only in form().
template <bool HARM, bool BC = false>
struct DivOp {
  static constexpr bool kFaces = true;
  double omega, g[kRelaxR], w[kRelaxR], cE[kRelaxR], cW[kRelaxR], cV[kRelaxR + 1];
  __device__ __forceinline__ explicit DivOp(double wt) : omega(wt) {}
  static __device__ __forceinline__ double rhs(double f, double, double inv_h2) { return f / inv_h2; }

  // the coefficient of the face between positions a and b (theta 1 is staged outside the grid: the mean is finite)
  static __device__ __forceinline__ double face(double ta, double tb, bool in_a, bool in_b) {
    const double m = face_mean<HARM>(ta, tb);
    return in_a && in_b ? m : (in_a ? ta : tb);
  }
  // ghost_a: the ghost face that a has when b is outside the grid exists (that side is Dirichlet); ghost_b likewise
  static __device__ __forceinline__ double face(double ta, double tb, bool in_a, bool in_b, bool ghost_a,
                                                bool ghost_b) {
    const double m = face_mean<HARM>(ta, tb);
    return in_a && in_b ? m : (in_a ? (ghost_a ? ta : 0.0) : (in_b ? (ghost_b ? tb : 0.0) : tb));
  }

  // the faces and w of the thread's strip from the staged theta plane
  __device__ __forceinline__ void form(const double* th, int x, int y0, int gx, int gy0, int n, int bc) {
    constexpr int P = kRelaxP, R = kRelaxR;
    // the outside end of a one-ended face lies above row 0 (N), below row n - 1 (S), left of column 0 (W) or right of
    // column n - 1 (E); at a patch edge the rule also meets in-grid ends, on positions that are never live
    const bool gh_n = !(bc & 1), gh_s = !(bc & 2), gh_w = !(bc & 4), gh_e = !(bc & 8);
    const bool col_in = gx >= 0 && gx < n, col_in_e = gx + 1 >= 0 && gx + 1 < n;
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
      if constexpr (BC) {
        cV[r] = face(tc, t_prev, in_c, in_prev, gh_n, gh_s);
        cE[r] = face(tc, te, in_c, col_in_e && row_in && x + 1 < P, gh_e, gh_w);
      } else {
        cV[r] = face(tc, t_prev, in_c, in_prev);
        cE[r] = face(tc, te, in_c, col_in_e && row_in && x + 1 < P);
      }
      t_prev = tc;
      in_prev = in_c;
    }
    const bool below_in = y0 + R < P && col_in && gy0 + R >= 0 && gy0 + R < n;
    const double t_below = y0 + R < P ? th[(y0 + R) * P + x] : 1.0;
    if constexpr (BC)
      cV[R] = face(t_prev, t_below, in_prev, below_in, gh_s, gh_n);
    else
      cV[R] = face(t_prev, t_below, in_prev, below_in);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cW[r] = __shfl_up(cE[r], 1, 64);                 // lane 0 keeps its own: patch column 0 is never live
      w[r] = omega / ((cE[r] + cW[r]) + (cV[r + 1] + cV[r]));
    }
  }

  __device__ __forceinline__ double update(int r, double cur, double prev, double dn, double uW, double uE) const {
    const double a = (cE[r] * (uE - cur) + cW[r] * (uW - cur)) + (cV[r + 1] * (dn - cur) + cV[r] * (prev - cur));
    return cur + w[r] * (a - g[r]);
  }
};

// grid (tiles, tiles, E); ks <= K sweeps from u_in to u_out (ks = 0: a copy); wt: 0.25 * omega (PointwiseOp) or omega;
// bc: the side mask, read by DivOp<HARM, true> alone.  The body of relax_kernel and relax_bd_kernel.
// BD (srpde_div_relax_bd, with DivOp<HARM, true>): bd is the example's boundary data (div_stencil.h).  Staging alone
// differs: an out-of-grid position straight beyond a Dirichlet side's edge node holds g instead of 0 -- it is fixed, so
// it keeps g through every sweep -- and a node on a flux side forms its right-hand-side register as
// g = (f - ((qE + qW) + (qS + qN)) * inv_h) / inv_h2.  The sweep loop is the same code.
template <class Op, bool BD = false>
__device__ __forceinline__ void relax_tile(const double* __restrict__ u_in, const double* __restrict__ f,
                                           const double* __restrict__ theta, double* __restrict__ u_out, int n,
                                           double inv_h2, double wt, int ks, int interior_only, int bc,
                                           const double* __restrict__ bd = nullptr, double inv_h = 0.0) {
  constexpr int P = kRelaxP, K = kRelaxK, T = kRelaxT, R = kRelaxR;
  __shared__ double plane[2][P * P];
  const int x = threadIdx.x & 63, y0 = (threadIdx.x >> 6) * R;
  const int gx = (int)blockIdx.x * T - K + x, gy0 = (int)blockIdx.y * T - K + y0;
  const long long base = (long long)blockIdx.z * n * n;
  const bool col_in = gx >= 0 && gx < n;
  const bool col_fixed = !col_in || (interior_only && (gx == 0 || gx == n - 1));

  Op op(wt);
  double uc[R];
  unsigned fixed = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gy = gy0 + r;
    const bool row_in = gy >= 0 && gy < n;
    double uv = 0.0, gv = 0.0, tv = 1.0;
    if (col_in && row_in) {
      const long long k = base + (long long)gy * n + gx;
      uv = u_in[k];
      double fv = f[k];
      tv = theta[k];
      if (BD && bd_flux_node(gy, gx, n, bc)) fv = fv - bd_flux_sum(bd, gy, gx, n, bc) * inv_h;
      gv = Op::rhs(fv, tv, inv_h2);
    }
    uc[r] = uv;
    op.g[r] = gv;
    if (col_fixed || !row_in || (interior_only && (gy == 0 || gy == n - 1))) fixed |= 1u << r;
    plane[0][(y0 + r) * P + x] = uv;
    if constexpr (Op::kFaces) plane[1][(y0 + r) * P + x] = tv;
  }
  if constexpr (BD) {
    // the ghost values go through the plane, in a loop that is not unrolled (its row tests are scalar and would
    // otherwise be live for all R rows at once), and come back into uc with the strip's own positions below
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
      const int gy = gy0 + r;
      if (!(col_in && gy >= 0 && gy < n)) plane[0][(y0 + r) * P + x] = bd_halo(bd, gy, gx, n, bc);
    }
  }
  __syncthreads();
  if constexpr (BD) {
#pragma unroll
    for (int r = 0; r < R; ++r) uc[r] = plane[0][(y0 + r) * P + x];
  }
  if constexpr (Op::kFaces) {
    op.form(plane[1], x, y0, gx, gy0, n, bc);
    __syncthreads();                                   // sweep 1 writes the plane theta was staged in
  }

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
        const double nv = (fixed >> r) & 1u ? cur : op.update(r, cur, prev, dn, uW, uE);
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

template <class Op>
__global__ __launch_bounds__(kRelaxThreads) void relax_kernel(const double* __restrict__ u_in,
                                                              const double* __restrict__ f,
                                                              const double* __restrict__ theta,
                                                              double* __restrict__ u_out, int n, double inv_h2,
                                                              double wt, int ks, int interior_only, int bc) {
  relax_tile<Op>(u_in, f, theta, u_out, n, inv_h2, wt, ks, interior_only, bc);
}

// bd_stride: 4 n, or 0 for one [4][n] shared by every example
template <class Op>
__global__ __launch_bounds__(kRelaxThreads) void relax_bd_kernel(const double* __restrict__ u_in,
                                                                 const double* __restrict__ f,
                                                                 const double* __restrict__ theta,
                                                                 double* __restrict__ u_out, int n, double inv_h2,
                                                                 double wt, int ks, int bc,
                                                                 const double* __restrict__ bd, long long bd_stride,
                                                                 double inv_h) {
  relax_tile<Op, true>(u_in, f, theta, u_out, n, inv_h2, wt, ks, 0, bc, bd + (long long)blockIdx.z * bd_stride, inv_h);
}

using RelaxKernel = decltype(&relax_kernel<PointwiseOp>);
using RelaxBdKernel = decltype(&relax_bd_kernel<DivOp<true, true>>);

inline bool relax_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p < q + bytes && q < p + bytes;
}

size_t relax_workspace_size(int E, int n, int sweeps) {
  if (E <= 0 || n < 1 || sweeps <= kRelaxK) return 0;
  return (size_t)E * n * n * sizeof(double);
}

// the checks and launches of both entries; name: the entry's, kernel and wt: its relax_kernel instance and weight,
// face_mean: the divergence entries' argument (checked in its place among the others), null for the pointwise entry;
// bc: srpde_div_relax_bc's side mask, 0 for the other entries; bd_kernel (srpde_div_relax_bd): launched in place of
// kernel, with the boundary data bd / bd_stride
int relax_run(const char* name, RelaxKernel kernel, double wt, const int* face_mean, const double* u_in,
              const double* f, const double* theta, double* u_out, int E, int n, double inv_h2, int sweeps, double omega,
              int interior_only, void* workspace, size_t ws_bytes, hipStream_t stream, int bc = 0,
              RelaxBdKernel bd_kernel = nullptr, const double* bd = nullptr, long long bd_stride = 0) {
  SRPDE_CHECK_ARG(u_in && f && theta && u_out, "%s: null pointer", name);
  if (E <= 0 || E > 65535 || n < 1 || n > kRelaxMaxN || (interior_only && n < 3))
    SRPDE_FAIL(kErrShape, "%s: bad shape E=%d n=%d (1 <= E <= 65535, 1 <= n <= %d, interior_only needs n >= 3)", name,
               E, n, kRelaxMaxN);
  if (face_mean && *face_mean != 0 && *face_mean != 1)
    SRPDE_FAIL(kErrArg, "%s: face_mean=%d (0 arithmetic, 1 harmonic)", name, *face_mean);
  if (bc < 0 || bc > 15)
    SRPDE_FAIL(kErrArg, "%s: bc=%d is not a side mask (bits 0..3: row 0, row n-1, column 0, column n-1; set = zero flux)",
               name, bc);
  if (bc && interior_only)
    SRPDE_FAIL(kErrArg, "%s: bc=%d with interior_only: the ring is held and no ghost face is read", name, bc);
  if (bc && n < 2)
    SRPDE_FAIL(kErrShape, "%s: bc=%d needs n >= 2 (a lone node's face coefficients can all be 0)", name, bc);
  if (bd_kernel) {
    if (!bd) SRPDE_FAIL(kErrArg, "%s: null boundary data", name);
    if (reinterpret_cast<uintptr_t>(bd) & 7u) SRPDE_FAIL(kErrAlign, "%s: bd not 8-byte aligned", name);
    if (bd_stride != 0 && bd_stride != 4LL * n)
      SRPDE_FAIL(kErrArg, "%s: bd_stride=%lld is neither 4 n = %lld ([E][4][n]) nor 0 (one [4][n] for every example)",
                 name, bd_stride, 4LL * n);
    if (n < 2) SRPDE_FAIL(kErrShape, "%s: boundary data needs n >= 2 (a side has an edge node per end)", name);
  }
  if (sweeps < 0) SRPDE_FAIL(kErrArg, "%s: sweeps=%d is negative", name, sweeps);
  if (!(omega > 0.0 && omega <= 1.0)) SRPDE_FAIL(kErrArg, "%s: omega=%g outside (0, 1]", name, omega);
  if (!(inv_h2 > 0.0) || !std::isfinite(inv_h2))
    SRPDE_FAIL(kErrArg, "%s: inv_h2=%g must be positive and finite", name, inv_h2);
  const size_t bytes = (size_t)E * n * n * sizeof(double);
  const size_t need = relax_workspace_size(E, n, sweeps);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(u_in) | reinterpret_cast<uintptr_t>(f) |
                         reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(u_out) |
                         (need ? reinterpret_cast<uintptr_t>(workspace) : 0);
  if (bits & 7u) SRPDE_FAIL(kErrAlign, "%s: a pointer is not 8-byte aligned", name);
  if (relax_overlap(u_out, u_in, bytes) || relax_overlap(u_out, f, bytes) || relax_overlap(u_out, theta, bytes))
    SRPDE_FAIL(kErrArg, "%s: u_out overlaps an input (a sweep reads its neighbours' old values)", name);
  if (need) {
    if (workspace == nullptr || ws_bytes < need) SRPDE_FAIL(kErrWorkspace, "%s: workspace too small", name);
    if (relax_overlap(workspace, u_out, bytes) || relax_overlap(workspace, u_in, bytes) ||
        relax_overlap(workspace, f, bytes) || relax_overlap(workspace, theta, bytes))
      SRPDE_FAIL(kErrArg, "%s: the workspace overlaps a field", name);
  }
  const int tiles = ceil_div(n, kRelaxT);
  const int launches = std::max(1, ceil_div(sweeps, kRelaxK));
  double* ws = static_cast<double*>(workspace);
  const double* src = u_in;
  for (int j = 0; j < launches; ++j) {
    // the last launch writes u_out, the one before it the workspace, and so on backwards
    double* dst = ((launches - 1 - j) & 1) ? ws : u_out;
    const int ks = std::min(kRelaxK, sweeps - j * kRelaxK);
    if (bd_kernel)
      hipLaunchKernelGGL(bd_kernel, dim3(tiles, tiles, E), dim3(kRelaxThreads), 0, stream, src, f, theta, dst, n, inv_h2,
                         wt, ks, bc, bd, bd_stride, std::sqrt(inv_h2));
    else
      hipLaunchKernelGGL(kernel, dim3(tiles, tiles, E), dim3(kRelaxThreads), 0, stream, src, f, theta, dst, n, inv_h2,
                         wt, ks, interior_only, bc);
    SRPDE_LAUNCH_CHECK(name);
    src = dst;
  }
  return 0;
}

}  // namespace
}  // namespace srpde

using namespace srpde;

extern "C" {

int srpde_pde_relax_sweeps_per_launch(void) { return kRelaxK; }

size_t srpde_pde_relax_workspace_size(int E, int n, int sweeps) { return relax_workspace_size(E, n, sweeps); }
size_t srpde_div_relax_workspace_size(int E, int n, int sweeps) { return relax_workspace_size(E, n, sweeps); }

int srpde_pde_relax(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                    double inv_h2, int sweeps, double omega, int interior_only, void* workspace, size_t ws_bytes,
                    hipStream_t stream) {
  return relax_run("srpde_pde_relax", relax_kernel<PointwiseOp>, 0.25 * omega, nullptr, u_in, f, theta, u_out, E, n,
                   inv_h2, sweeps, omega, interior_only, workspace, ws_bytes, stream);
}

int srpde_div_relax(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                    int face_mean, double inv_h2, int sweeps, double omega, int interior_only, void* workspace,
                    size_t ws_bytes, hipStream_t stream) {
  return relax_run("srpde_div_relax", face_mean == 1 ? relax_kernel<DivOp<true>> : relax_kernel<DivOp<false>>, omega,
                   &face_mean, u_in, f, theta, u_out, E, n, inv_h2, sweeps, omega, interior_only, workspace, ws_bytes,
                   stream);
}

// bc = 0 is srpde_div_relax, kernel for kernel
int srpde_div_relax_bc(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                       int face_mean, int bc, double inv_h2, int sweeps, double omega, int interior_only,
                       void* workspace, size_t ws_bytes, hipStream_t stream) {
  RelaxKernel kernel = face_mean == 1 ? relax_kernel<DivOp<true>> : relax_kernel<DivOp<false>>;
  if (bc != 0) kernel = face_mean == 1 ? relax_kernel<DivOp<true, true>> : relax_kernel<DivOp<false, true>>;
  return relax_run("srpde_div_relax_bc", kernel, omega, &face_mean, u_in, f, theta, u_out, E, n, inv_h2, sweeps, omega,
                   interior_only, workspace, ws_bytes, stream, bc);
}

// srpde_div_relax_bc with boundary data: bc = 0 is four Dirichlet sides with values; no interior_only
int srpde_div_relax_bd(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                       int face_mean, int bc, double inv_h2, int sweeps, double omega, const double* bd,
                       long long bd_stride, void* workspace, size_t ws_bytes, hipStream_t stream) {
  return relax_run("srpde_div_relax_bd", nullptr, omega, &face_mean, u_in, f, theta, u_out, E, n, inv_h2, sweeps, omega,
                   0, workspace, ws_bytes, stream, bc,
                   face_mean == 1 ? relax_bd_kernel<DivOp<true, true>> : relax_bd_kernel<DivOp<false, true>>, bd,
                   bd_stride);
}

}  // extern "C"
