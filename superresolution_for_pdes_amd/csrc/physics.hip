// The discrete equation as a loss term and as an evaluation metric, gfx950.
//
// Every training sample is a solution of  theta * L u = f  on an n x n grid, L = A / h^2 with A the 5-point
// stencil (sum of the four neighbours minus 4x the centre).  From the normalised fields the model sees
// (y = (u - mu_u) / sigma_u, x1 = (theta - mu_t) / sigma_t, x2 = (f - mu_f) / sigma_f) the residual is
//
//     r = (theta * (sigma_u * A y + mu_u * A 1) / h^2 - f) / sigma_f
//
// in this split form: A y is a difference of O(1) numbers and A 1 = -(number of missing neighbours) is exact, so
// nothing of the size of mu_u / h^2 is ever added to and subtracted from a single fp32 value.
//   kind 0 (whole-domain solve): zero ghost ring outside the grid, all n^2 nodes counted;
//   kind 1 (crop of a finer solve): the ring outside the crop is unknown, so only the (n - 2)^2 interior nodes
//          are counted (the mask m); the crop's own boundary nodes still enter as neighbours.
// The two 1 / h^2 values are arguments.
//
//   srpde_physics_loss_fwd   loss = mean((y - t)^2) + weight * sum(m r^2) / sum(m)             [2 launches]
//                            and, when asked, the gradient for grad_out = 1:
//                            dy = 2 (y - t) / N + weight * (2 sigma_u / (M sigma_f h^2)) A(m r theta)
//   srpde_physics_loss_bwd   dy = grad_out * that                                                [1 launch]
//   srpde_pde_residual_metrics  per example (RMS, max |.|) of theta * A u / h^2 - f in fp64     [2 launches]
//
// Loss kernel: a workgroup takes spw consecutive samples.  Their y planes are staged in LDS with a zero halo
// (pitch n + 2), so the stencil needs no bounds test; q = m r theta goes to a second halo tile and y - t to a
// third plane, so the adjoint (A is symmetric: the same stencil on q) is formed after one barrier without reading
// global memory again.  y, t, theta and f are each read once.  M = sum(m) follows from the kinds alone, so every
// workgroup counts it from kind[] (integers, the same value everywhere) and the gradient needs no second pass.
// Each workgroup leaves fp64 partials {sum (y - t)^2, sum m r^2, sum m}; one block adds them in index order.  The
// node -> thread -> workgroup assignment depends on the shape alone and there are no atomics: results are
// bit-reproducible.
#include "common.h"
#include "div_stencil.h"
#include "field_reduce.h"

namespace srpde {
namespace {

constexpr int kPhysThreads = 256;
constexpr int kPhysMaxSpw = 2;            // samples per workgroup, LDS permitting
constexpr int kPhysLdsBudget = 48 * 1024;
constexpr int kPhysMinN = 3, kPhysMaxN = 64;

inline int phys_spw(size_t lds_floats) {
  const size_t per = lds_floats * sizeof(float);
  return (int)std::max<size_t>(1, std::min<size_t>(kPhysMaxSpw, kPhysLdsBudget / per));
}
inline int phys_blocks(int B, size_t lds_floats) { return ceil_div(B, phys_spw(lds_floats)); }

// (a + b) + (c + d) - 4 e on a halo tile around p
__device__ __forceinline__ float stencil5(const float* p, int pitch) {
  return fmaf(-4.f, p[0], (p[-pitch] + p[pitch]) + (p[-1] + p[1]));
}

// ---- the two operators of the loss term ----------------------------------------------------------------------------
// physics_loss_kernel<Op> owns the sample-to-workgroup mapping, the two passes over the nodes, the count of M, the fp64
// accumulation, the gradient's scale constants and the partials.  What an operator does differently -- its LDS layout,
// what it stages beside y, its residual at a node, what the node leaves in LDS for the gradient pass and its adjoint
// stencil -- stands in the kernel under `if constexpr (Op::kDiv)`, each operator's statements in the order and with the
// index forms its own kernel had, so that each instance compiles as that kernel did.
//
// theta * L (the header's formulas): q = m r theta, the adjoint is A on q.  LDS per sample: the y and q halo tiles and
// the y - t plane.
struct PointwiseLoss {
  static constexpr bool kDiv = false, kBd = false;
  static size_t lds_floats(int n) { return 2 * (size_t)(n + 2) * (n + 2) + (size_t)n * n; }
};

// div(theta grad u) - f: D_theta (sigma_u y + mu_u) = sigma_u a(y) + mu_u D_theta 1, with a(y) the face sum of
// div_stencil.h on y (zero halo, ghost coefficient theta_a) and D_theta 1 = -(sum of the node's ghost-face
// coefficients) = -k_miss theta, because the interior faces cancel: the same split as above, nothing of the size of
// mu_u / h^2 enters an fp32 sum.
//     r  = ((sigma_u a(y) + mu_u (-k_miss theta)) ih2 - f) / sigma_f
//     dy = 2 (y - t) / N + weight (2 sigma_u / (M sigma_f)) ih2 Dt(q),   q = m r
// Dt is the face operator with the ghost faces on the diagonal; it is symmetric, so the adjoint is the same face sum
// on q (q, not q theta: theta sits in the faces).  LDS per sample: the y, theta and q halo tiles, 3 (n + 2)^2 floats
// -- 51 KiB at n = 64, one sample per workgroup there, inside the 64 KiB that a kernel gets without raising its limit.
// The y - t plane is not kept: the gradient pass reads t again (the workgroup's own lines, just read).  theta's halo
// is 1: every face towards it is replaced by the ghost rule, so the mean never divides by 0.
//
// BC (srpde_physics_loss_div_fwd_bc): with the side mask bc (bit 0 the row 0 side, 1 row n - 1, 2 column 0, 3 column
// n - 1; set: zero flux) on the kind-0 samples.  The residual and the adjoint take face_sum_bc -- the operator with
// missing ghost faces is still symmetric -- and D_theta 1 = -k_d theta, k_d the number of the node's Dirichlet ghost
// faces.  A kind-1 sample counts interior nodes only: its m r is 0 on the ring, so no ghost coefficient reaches its
// loss or its gradient, and it is computed with mask 0, as DivLoss<HARM, false> computes it.
//
// BD (srpde_physics_loss_div_fwd_bd): boundary data on the kind-0 samples, raw units, [4][n] floats per sample in the
// mask's side order: the ghost value g beyond a Dirichlet side, the outward flux q through a flux side.  The operator
// gains the affine term b of srpde_div_apply_bd, which does not depend on y:
//     r = ((((sigma_u a(y) + mu_u (-k_d theta)) + beta) ih2 - f) + Q inv_h) / sigma_f
// beta = (tE + tW) + (tS + tN), a term theta_a * g for a Dirichlet ghost face and 0.0 otherwise; Q = (qE + qW) +
// (qS + qN), added at nodes with a flux-side ghost face only.  The line that forms (.) ih2 - f is the one every
// instance shares, so zero data gives the BC instance's numbers.  The gradient is Dt(m r) with this r, the adjoint pass
// untouched.  The kind-0 samples' data is staged once into 4 n floats of LDS behind the three tiles (a crop's row is
// neither loaded nor read); the tiles, the samples per workgroup (still chosen from the three tiles alone), the
// partials and the workspace are the BC instance's: 52 KiB at n = 64.
template <bool HARM, bool BC = false, bool BD = false>
struct DivLoss {
  static_assert(BC || !BD, "boundary data rides on the instance with a side mask (mask 0: four Dirichlet sides)");
  static constexpr bool kDiv = true, kHarm = HARM, kBc = BC, kBd = BD;
  static size_t lds_floats(int n) { return 3 * (size_t)(n + 2) * (n + 2); }
};

// the face sum of node (i, j) on halo tiles around v and th
template <bool HARM>
__device__ __forceinline__ float loss_face_sum(const float* v, const float* th, int pitch, int i, int j, int n) {
  return face_sum<HARM>(v, th, pitch, j > 0, j < n - 1, i > 0, i < n - 1);
}
template <bool HARM>
__device__ __forceinline__ float loss_face_sum_bc(const float* v, const float* th, int pitch, int i, int j, int n,
                                                  int bc) {
  return face_sum_bc<HARM>(v, th, pitch, j > 0, j < n - 1, i > 0, i < n - 1, !(bc & 4), !(bc & 8), !(bc & 1),
                           !(bc & 2));
}

// what differs between DivLoss<HARM, false> and <HARM, true> at a node: the face sum, and the number of its ghost
// faces that exist (all of the missing neighbours without a mask; those on ghost-ring sides with the mask sb)
template <class Op>
__device__ __forceinline__ float loss_face_sum_op(const float* v, const float* th, int pitch, int i, int j, int n,
                                                  int sb) {
  if constexpr (Op::kBc)
    return loss_face_sum_bc<Op::kHarm>(v, th, pitch, i, j, n, sb);
  else
    return loss_face_sum<Op::kHarm>(v, th, pitch, i, j, n);
}
template <class Op>
__device__ __forceinline__ int loss_ghost_count(int miss, int i, int j, int n, int sb) {
  if constexpr (Op::kBc)
    return (i == 0 && !(sb & 1)) + (i == n - 1 && !(sb & 2)) + (j == 0 && !(sb & 4)) + (j == n - 1 && !(sb & 8));
  else
    return miss;
}

// grid: ceil(B / spw) workgroups; dynamic LDS: spw * Op::lds_floats(n) floats (kBd: + spw * 4 n for the walls); bc: the
// side mask, read by DivLoss<HARM, true> alone; bd [Bd][4][n], bd_stride (4 n or 0) and inv_h: read by
// DivLoss<HARM, true, true> alone
template <class Op>
__global__ __launch_bounds__(kPhysThreads) void physics_loss_kernel(
    const float* __restrict__ y, const float* __restrict__ t, const float* __restrict__ x,
    const int* __restrict__ kind, const float* __restrict__ stats, int B, int n, int spw, float weight, float ih2_std,
    float ih2_sub, float* __restrict__ dy, double* __restrict__ part, int bc, const float* __restrict__ bd,
    long long bd_stride, float inv_h) {
  extern __shared__ float lds[];
  __shared__ double sh[4];
  __shared__ long long shM;
  const int tid = threadIdx.x;
  const int P = n + 2, T2 = P * P, nn = n * n;
  const int b0 = blockIdx.x * spw;
  const int ns = min(spw, B - b0);            // samples of this workgroup (>= 1)
  float* ytile = lds;                         // [spw][P][P]
  float* tile2 = lds + (size_t)spw * T2;      // [spw][P][P]: q (pointwise), theta (divergence)
  float* tile3 = tile2 + (size_t)spw * T2;    // [spw][n][n] y - t (pointwise), [spw][P][P] q (divergence)
  float* ttile = tile2;
  float* qtile = Op::kDiv ? tile3 : tile2;
  float* dpl = tile3;

  const float mu_u = stats[0], sg_u = stats[1], mu_f = stats[2], sg_f = stats[3], mu_t = stats[4], sg_t = stats[5];

  // stage y with its zero halo (divergence: and theta with a halo of 1); zero q's halo
  for (int k = tid; k < ns * T2; k += kPhysThreads) {
    const int s = k / T2, rem = k - s * T2;
    const int ii = rem / P, jj = rem - ii * P;
    const bool inner = ii >= 1 && ii <= n && jj >= 1 && jj <= n;
    if constexpr (Op::kDiv) {
      float v = 0.f, th = 1.f;
      if (inner) {
        const long long at = (long long)(ii - 1) * n + (jj - 1);
        v = y[(long long)(b0 + s) * nn + at];
        th = fmaf(sg_t, x[((long long)(b0 + s) * 3 + 1) * nn + at], mu_t);
      }
      ytile[k] = v;
      ttile[k] = th;
    } else {
      float v = 0.f;
      if (inner) v = y[(long long)(b0 + s) * nn + (ii - 1) * n + (jj - 1)];
      ytile[k] = v;
    }
    if (!inner) qtile[k] = 0.f;
  }
  // stage the walls of the kind-0 samples behind the tiles, once
  [[maybe_unused]] float* wall = tile3 + (size_t)spw * T2;   // [spw][4][n] (boundary data only)
  if constexpr (Op::kBd) {
    const int W = 4 * n;
    for (int k = tid; k < ns * W; k += kPhysThreads) {
      const int s = k / W;
      wall[k] = kind[b0 + s] ? 0.f : bd[(long long)(b0 + s) * bd_stride + (k - s * W)];
    }
  }
  // M = sum of the masks of the whole batch, from the kinds (only the gradient's scale needs it here)
  if (dy != nullptr) {
    long long cnt = 0;
    for (int b = tid; b < B; b += kPhysThreads) cnt += kind[b] ? (long long)(n - 2) * (n - 2) : (long long)nn;
    const double tot = block_sum((double)cnt, sh);   // exact: integers far below 2^53
    if (tid == 0) shM = (long long)tot;
  }
  __syncthreads();

  double sse = 0.0, spr = 0.0, sm = 0.0;
  for (int k = tid; k < ns * nn; k += kPhysThreads) {
    const int s = k / nn, rem = k - s * nn;
    const int i = rem / n, j = rem - i * n;
    const long long b = b0 + s;
    float r, d, qv;                           // the residual, y - t and what goes into q if the node is counted
    bool m;
    if constexpr (Op::kDiv) {
      const int c = s * T2 + (i + 1) * P + (j + 1);
      const float f = fmaf(sg_f, x[(b * 3 + 2) * nn + rem], mu_f);
      const float tv = t[b * nn + rem];
      const int kd = kind[b];
      const float ih2 = kd ? ih2_sub : ih2_std;
      const int sb = Op::kBc && !kd ? bc : 0;   // a crop's ring is never counted: no pattern there
      const float ay = loss_face_sum_op<Op>(ytile + c, ttile + c, P, i, j, n, sb);
      const int miss = (i == 0) + (i == n - 1) + (j == 0) + (j == n - 1);
      m = !kd || miss == 0;
      const float d1 = -(float)loss_ghost_count<Op>(miss, i, j, n, sb) * ttile[c];
      float lap = fmaf(sg_u, ay, mu_u * d1);
      float qh = 0.f;                           // Q inv_h of a node with a flux-side ghost face
      if constexpr (Op::kBd) {
        if (!kd && miss) {                      // an edge node of a whole-domain sample
          const float* w = wall + s * 4 * n;
          const float ta = ttile[c];
          const bool eN = i == 0, eS = i == n - 1, eW = j == 0, eE = j == n - 1;
          const float tN = eN && !(sb & 1) ? ta * w[j] : 0.f, tS = eS && !(sb & 2) ? ta * w[n + j] : 0.f;
          const float tW = eW && !(sb & 4) ? ta * w[2 * n + i] : 0.f, tE = eE && !(sb & 8) ? ta * w[3 * n + i] : 0.f;
          lap += (tE + tW) + (tS + tN);
          const float qN = eN && (sb & 1) ? w[j] : 0.f, qS = eS && (sb & 2) ? w[n + j] : 0.f;
          const float qW = eW && (sb & 4) ? w[2 * n + i] : 0.f, qE = eE && (sb & 8) ? w[3 * n + i] : 0.f;
          if ((eN && (sb & 1)) || (eS && (sb & 2)) || (eW && (sb & 4)) || (eE && (sb & 8)))
            qh = ((qE + qW) + (qS + qN)) * inv_h;
        }
      }
      float num = lap * ih2 - f;
      if constexpr (Op::kBd) num += qh;
      r = num / sg_f;
      d = ytile[c] - tv;
      qv = r;
    } else {
      const long long g = b * nn + rem;
      const float* xb = x + b * 3 * nn + rem;
      const float th = fmaf(sg_t, xb[nn], mu_t);
      const float f = fmaf(sg_f, xb[2 * nn], mu_f);
      const float tv = t[g];
      const int kd = kind[b];
      const float ih2 = kd ? ih2_sub : ih2_std;
      const float* yc = ytile + s * T2 + (i + 1) * P + (j + 1);
      const float ay = stencil5(yc, P);
      const int edge_i = (i == 0) + (i == n - 1), edge_j = (j == 0) + (j == n - 1);
      const float a1 = -(float)(edge_i + edge_j);
      m = !kd || (edge_i + edge_j == 0);
      const float lap = fmaf(sg_u, ay, mu_u * a1);
      r = (th * lap * ih2 - f) / sg_f;
      d = yc[0] - tv;
      qv = r * th;
    }
    sse += (double)(d * d);
    if (m) {
      spr += (double)r * (double)r;
      sm += 1.0;
    }
    if (dy != nullptr) {
      qtile[s * T2 + (i + 1) * P + (j + 1)] = m ? qv : 0.f;
      if constexpr (!Op::kDiv) dpl[k] = d;
    }
  }

  if (dy != nullptr) {
    __syncthreads();
    const double M = (double)shM;
    const double base = 2.0 * (double)weight * (double)sg_u / (M * (double)sg_f);
    const float c_std = (float)(base * (double)ih2_std), c_sub = (float)(base * (double)ih2_sub);
    const float c_mse = (float)(2.0 / ((double)B * (double)nn));
    for (int k = tid; k < ns * nn; k += kPhysThreads) {
      const int s = k / nn, rem = k - s * nn;
      const int i = rem / n, j = rem - i * n;
      const long long b = b0 + s;
      if constexpr (Op::kDiv) {
        const int c = s * T2 + (i + 1) * P + (j + 1);
        const float aq = loss_face_sum_op<Op>(qtile + c, ttile + c, P, i, j, n, Op::kBc && !kind[b] ? bc : 0);
        const float d = ytile[c] - t[b * nn + rem];
        dy[b * nn + rem] = fmaf(kind[b] ? c_sub : c_std, aq, c_mse * d);
      } else {
        const float aq = stencil5(qtile + s * T2 + (i + 1) * P + (j + 1), P);
        dy[b * nn + rem] = fmaf(kind[b] ? c_sub : c_std, aq, c_mse * dpl[k]);
      }
    }
  }

  sse = block_sum(sse, sh);
  spr = block_sum(spr, sh);
  sm = block_sum(sm, sh);
  if (tid == 0) {
    double* o = part + (long long)blockIdx.x * 3;
    o[0] = sse;
    o[1] = spr;
    o[2] = sm;
  }
}

// one block: loss = {mse + weight * pde, mse, pde}
__global__ __launch_bounds__(kPhysThreads) void physics_loss_final_kernel(const double* __restrict__ part, int nblk,
                                                                           long long N, float weight,
                                                                           float* __restrict__ loss) {
  __shared__ double sh[4];
  double a = 0.0, b = 0.0, c = 0.0;
  for (int k = threadIdx.x; k < nblk; k += kPhysThreads) {
    a += part[3 * (long long)k];
    b += part[3 * (long long)k + 1];
    c += part[3 * (long long)k + 2];
  }
  a = block_sum(a, sh);
  b = block_sum(b, sh);
  c = block_sum(c, sh);
  if (threadIdx.x == 0) {
    const double mse = a / (double)N, pde = b / c;
    loss[0] = (float)(mse + (double)weight * pde);
    loss[1] = (float)mse;
    loss[2] = (float)pde;
  }
}

__global__ void physics_scale_kernel(const float* __restrict__ unit, long long n, const float* __restrict__ gout,
                                     float* __restrict__ dy) {
  const float g = gout ? gout[0] : 1.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dy[i] = unit[i] * g;
}

// ---- the residual metric ---------------------------------------------------------------------------------
// grid (red_blocks, E): part[(e * nb + b) * 2] = {sum r^2, max |r|} over the counted nodes.  Every operation is
// rounded on its own (no contraction), in the order of the header's formula, so a host restatement in that order
// reproduces r bit for bit.
template <typename TU>
__global__ __launch_bounds__(kRedThreads) void pde_residual_partial_kernel(const TU* __restrict__ u,
                                                                           const double* __restrict__ f,
                                                                           const double* __restrict__ theta, int n,
                                                                           double inv_h2, int interior_only,
                                                                           double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  const int e = blockIdx.y;
  const long long nn = (long long)n * n;
  const TU* ue = u + e * nn;
  const double* fe = f + e * nn;
  const double* te = theta + e * nn;
  double sq = 0.0, mx = 0.0;
  for (long long k = (long long)blockIdx.x * kRedThreads + threadIdx.x; k < nn; k += (long long)gridDim.x * kRedThreads) {
    const int i = (int)(k / n), j = (int)(k - (long long)i * n);
    const bool edge = i == 0 || i == n - 1 || j == 0 || j == n - 1;
    if (interior_only && edge) continue;
    const double up = i > 0 ? (double)ue[k - n] : 0.0, dn = i < n - 1 ? (double)ue[k + n] : 0.0;
    const double lf = j > 0 ? (double)ue[k - 1] : 0.0, rt = j < n - 1 ? (double)ue[k + 1] : 0.0;
    const double lap = ((up + dn) + (lf + rt)) - 4.0 * (double)ue[k];
    const double r = (te[k] * lap) * inv_h2 - fe[k];
    sq += r * r;
    mx = fmax(mx, fabs(r));
  }
  sq = block_sum(sq, sh);
  block_max_store(mx, sh);
  if (threadIdx.x == 0) {
    double* o = part + ((long long)e * gridDim.x + blockIdx.x) * 2;
    o[0] = sq;
    o[1] = block_max_load(sh);
  }
}

__global__ __launch_bounds__(64) void pde_residual_final_kernel(const double* __restrict__ part, int nb, double count,
                                                                double* __restrict__ out) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const double* p = part + (long long)e * nb * 2;
  double sq = 0.0, mx = 0.0;
  for (int j = lane; j < nb; j += 64) {
    sq += p[2 * j];
    mx = fmax(mx, p[2 * j + 1]);
  }
  sq = wave_sum(sq);
  mx = wave_max(mx);
  if (lane == 0) {
    out[e * 2] = sqrt(sq / count);
    out[e * 2 + 1] = mx;
  }
}

}  // namespace
}  // namespace srpde

using namespace srpde;

using PhysLossKernel = decltype(&srpde::physics_loss_kernel<srpde::PointwiseLoss>);

static size_t phys_workspace_size(int B, int n, size_t lds_floats) {
  if (B <= 0 || n < kPhysMinN || n > kPhysMaxN) return 0;
  return (size_t)phys_blocks(B, lds_floats) * 3 * sizeof(double);
}

// the checks and the two launches of both loss entries; name: the entry's, kernel and lds_floats: its operator's,
// face_mean: the divergence entries' argument (checked in its place among the others), null for the pointwise entry;
// bc: srpde_physics_loss_div_fwd_bc's side mask, 0 for the other entries; bd, bd_stride: srpde_physics_loss_div_fwd_bd's
// boundary data, null for the other entries
static int phys_loss_launch(const char* name, PhysLossKernel kernel, size_t lds_floats, const int* face_mean,
                            const float* y, const float* t, const float* x, const int* kind, const float* stats, int B,
                            int n, float weight, float inv_h2_std, float inv_h2_sub, float* loss, float* dy_unit,
                            void* workspace, size_t ws_bytes, hipStream_t stream, int bc = 0, const float* bd = nullptr,
                            long long bd_stride = 0) {
  SRPDE_CHECK_ARG(y && t && x && kind && stats && loss && workspace, "%s: null pointer", name);
  if (B <= 0 || n < kPhysMinN || n > kPhysMaxN)
    SRPDE_FAIL(kErrShape, "%s: bad shape B=%d n=%d (B >= 1, %d <= n <= %d)", name, B, n, kPhysMinN, kPhysMaxN);
  if (face_mean && *face_mean != 0 && *face_mean != 1)
    SRPDE_FAIL(kErrArg, "%s: face_mean=%d (0 arithmetic, 1 harmonic)", name, *face_mean);
  if (bc < 0 || bc > 15)
    SRPDE_FAIL(kErrArg, "%s: bc=%d is not a side mask (bits 0..3: row 0, row n-1, column 0, column n-1; set = zero flux)",
               name, bc);
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) SRPDE_FAIL(kErrAlign, "%s: workspace not 8-byte aligned", name);
  if (ws_bytes < phys_workspace_size(B, n, lds_floats)) SRPDE_FAIL(kErrWorkspace, "%s: workspace too small", name);
  if (bd && bd_stride != 0 && bd_stride != 4LL * n)
    SRPDE_FAIL(kErrArg, "%s: bd_stride=%lld (4 n = %d floats between samples, or 0 for one shared [4][n])", name,
               bd_stride, 4 * n);
  const int spw = phys_spw(lds_floats), nb = phys_blocks(B, lds_floats);
  const size_t lds = (size_t)spw * (lds_floats + (bd ? 4 * (size_t)n : 0)) * sizeof(float);
  const float inv_h = (float)sqrt((double)inv_h2_std);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(kPhysThreads), lds, stream, y, t, x, kind, stats, B, n, spw, weight,
                     inv_h2_std, inv_h2_sub, dy_unit, part, bc, bd, bd_stride, inv_h);
  SRPDE_LAUNCH_CHECK(name);
  hipLaunchKernelGGL(physics_loss_final_kernel, dim3(1), dim3(kPhysThreads), 0, stream, part, nb,
                     (long long)B * n * n, weight, loss);
  SRPDE_LAUNCH_CHECK(name);
  return 0;
}

extern "C" {

size_t srpde_physics_loss_workspace_size(int B, int n) {
  return phys_workspace_size(B, n, PointwiseLoss::lds_floats(n));
}

size_t srpde_physics_loss_div_workspace_size(int B, int n) {
  return phys_workspace_size(B, n, DivLoss<false>::lds_floats(n));
}

int srpde_physics_loss_fwd(const float* y, const float* t, const float* x, const int* kind, const float* stats, int B,
                           int n, float weight, float inv_h2_std, float inv_h2_sub, float* loss, float* dy_unit,
                           void* workspace, size_t ws_bytes, hipStream_t stream) {
  return phys_loss_launch("srpde_physics_loss_fwd", physics_loss_kernel<PointwiseLoss>, PointwiseLoss::lds_floats(n),
                          nullptr, y, t, x, kind, stats, B, n, weight, inv_h2_std, inv_h2_sub, loss, dy_unit, workspace,
                          ws_bytes, stream);
}

int srpde_physics_loss_div_fwd(const float* y, const float* t, const float* x, const int* kind, const float* stats,
                               int B, int n, int face_mean, float weight, float inv_h2_std, float inv_h2_sub,
                               float* loss, float* dy_unit, void* workspace, size_t ws_bytes, hipStream_t stream) {
  return phys_loss_launch("srpde_physics_loss_div_fwd",
                          face_mean == 1 ? physics_loss_kernel<DivLoss<true>> : physics_loss_kernel<DivLoss<false>>,
                          DivLoss<false>::lds_floats(n), &face_mean, y, t, x, kind, stats, B, n, weight, inv_h2_std,
                          inv_h2_sub, loss, dy_unit, workspace, ws_bytes, stream);
}

// bc = 0 is srpde_physics_loss_div_fwd, kernel for kernel
int srpde_physics_loss_div_fwd_bc(const float* y, const float* t, const float* x, const int* kind, const float* stats,
                                  int B, int n, int face_mean, int bc, float weight, float inv_h2_std,
                                  float inv_h2_sub, float* loss, float* dy_unit, void* workspace, size_t ws_bytes,
                                  hipStream_t stream) {
  PhysLossKernel kernel = face_mean == 1 ? physics_loss_kernel<DivLoss<true>> : physics_loss_kernel<DivLoss<false>>;
  if (bc != 0)
    kernel = face_mean == 1 ? physics_loss_kernel<DivLoss<true, true>> : physics_loss_kernel<DivLoss<false, true>>;
  return phys_loss_launch("srpde_physics_loss_div_fwd_bc", kernel, DivLoss<false>::lds_floats(n), &face_mean, y, t, x,
                          kind, stats, B, n, weight, inv_h2_std, inv_h2_sub, loss, dy_unit, workspace, ws_bytes, stream,
                          bc);
}

// bd == NULL is srpde_physics_loss_div_fwd_bc, kernel for kernel
int srpde_physics_loss_div_fwd_bd(const float* y, const float* t, const float* x, const int* kind, const float* stats,
                                  int B, int n, int face_mean, int bc, float weight, float inv_h2_std,
                                  float inv_h2_sub, const float* bd, long long bd_stride, float* loss, float* dy_unit,
                                  void* workspace, size_t ws_bytes, hipStream_t stream) {
  if (!bd)
    return srpde_physics_loss_div_fwd_bc(y, t, x, kind, stats, B, n, face_mean, bc, weight, inv_h2_std, inv_h2_sub,
                                         loss, dy_unit, workspace, ws_bytes, stream);
  return phys_loss_launch("srpde_physics_loss_div_fwd_bd",
                          face_mean == 1 ? physics_loss_kernel<DivLoss<true, true, true>>
                                         : physics_loss_kernel<DivLoss<false, true, true>>,
                          DivLoss<false>::lds_floats(n), &face_mean, y, t, x, kind, stats, B, n, weight, inv_h2_std,
                          inv_h2_sub, loss, dy_unit, workspace, ws_bytes, stream, bc, bd, bd_stride);
}

int srpde_physics_loss_bwd(const float* dy_unit, long long count, const float* gout, float* dy, hipStream_t stream) {
  SRPDE_CHECK_ARG(dy_unit && dy, "srpde_physics_loss_bwd: null pointer");
  if (count <= 0) SRPDE_FAIL(kErrShape, "srpde_physics_loss_bwd: bad count %lld", count);
  hipLaunchKernelGGL(physics_scale_kernel, dim3(elementwise_grid(count)), dim3(256), 0, stream, dy_unit, count, gout,
                     dy);
  SRPDE_LAUNCH_CHECK("srpde_physics_loss_bwd");
  return 0;
}

size_t srpde_pde_residual_metrics_workspace_size(int E, int n) {
  if (E <= 0 || n <= 0) return 0;
  return (size_t)E * red_blocks((long long)n * n) * 2 * sizeof(double);
}

int srpde_pde_residual_metrics(const void* u, int u_is_f32, const double* f, const double* theta, int E, int n,
                               double inv_h2, int interior_only, double* out, void* workspace, size_t ws_bytes,
                               hipStream_t stream) {
  SRPDE_CHECK_ARG(u && f && theta && out && workspace, "srpde_pde_residual_metrics: null pointer");
  if (E <= 0 || n <= 0 || E > 65535 || n > 16384 || (interior_only && n < 3))
    SRPDE_FAIL(kErrShape, "srpde_pde_residual_metrics: bad shape E=%d n=%d (interior_only needs n >= 3)", E, n);
  if (reinterpret_cast<uintptr_t>(workspace) & 7u)
    SRPDE_FAIL(kErrAlign, "srpde_pde_residual_metrics: workspace not 8-byte aligned");
  if (ws_bytes < srpde_pde_residual_metrics_workspace_size(E, n))
    SRPDE_FAIL(kErrWorkspace, "srpde_pde_residual_metrics: workspace too small");
  const long long nn = (long long)n * n;
  const int nb = red_blocks(nn);
  const double count = interior_only ? (double)(n - 2) * (n - 2) : (double)nn;
  double* part = static_cast<double*>(workspace);
  if (u_is_f32)
    hipLaunchKernelGGL(pde_residual_partial_kernel<float>, dim3(nb, E), dim3(kRedThreads), 0, stream,
                       static_cast<const float*>(u), f, theta, n, inv_h2, interior_only, part);
  else
    hipLaunchKernelGGL(pde_residual_partial_kernel<double>, dim3(nb, E), dim3(kRedThreads), 0, stream,
                       static_cast<const double*>(u), f, theta, n, inv_h2, interior_only, part);
  SRPDE_LAUNCH_CHECK("srpde_pde_residual_metrics");
  hipLaunchKernelGGL(pde_residual_final_kernel, dim3(E), dim3(64), 0, stream, part, nb, count, out);
  SRPDE_LAUNCH_CHECK("srpde_pde_residual_metrics");
  return 0;
}

}  // extern "C"
