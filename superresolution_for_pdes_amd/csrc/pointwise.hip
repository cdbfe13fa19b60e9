// Memory-bound U-Net ops for NHWC fp32 on gfx950: input staging, 2x2 max-pool,
// bilinear x2 upsample (align_corners=True), attention gate, output head + residual,
// MSE loss.  All reductions are deterministic (fixed-order partial sums, no atomics).
//
// Reference anchors (src/models.py): pool :69,:79-80; up :70,:89-93; AttentionGate
// :103-130; final 1x1 + residual :61,:74,:98,:101; nn.MSELoss src/train_enhanced.py:307.
#include "bn_reduce.h"

namespace srpde {

// ------------------------------- input staging ---------------------------------
// x NCHW [N][Cin][H][W] -> NHWC [N][H][W][Cpad] (extra channels zero)
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int Cin, int HW,
                                    int Cpad) {
  const long long total = (long long)N * HW;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long n = e / HW;
    const int p = (int)(e - n * HW);
    float* o = out + e * Cpad;
    for (int c = 0; c < Cpad; ++c) o[c] = c < Cin ? x[(n * Cin + c) * HW + p] : 0.f;
  }
}

// gradient w.r.t. the model input: NHWC rows [P, ldx] -> NCHW [N, C, HW] (first C channels)
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int N, int C,
                                    int HW) {
  const long long total = (long long)N * C * HW;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long nc = e / HW;
    const int p = (int)(e - nc * HW);
    const long long n = nc / C;
    const int c = (int)(nc - n * C);
    out[e] = x[(n * HW + p) * ldx + c];
  }
}

// y[n, ch, :] += alpha * x[n, :] for y [N, C, HW] (the residual x[:, 0:1] of models.py:74,101)
__global__ void axpy_channel_kernel(float* __restrict__ y, const float* __restrict__ x, int N, int C, int HW, int ch,
                                    float alpha) {
  const long long total = (long long)N * HW;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long n = e / HW;
    const int p = (int)(e - n * HW);
    y[(n * C + ch) * HW + p] += alpha * x[e];
  }
}

// Each vector op below has a grid-stride kernel (any C % 4 == 0: a 64-bit element index divided per float4) and a
// pixel-blocked one (C / 4 a power of two <= 256, further down); a pair shares one body, templated on the type I
// its pixel indices multiply in: long long, or the pixel-blocked kernels' size_t over 32-bit products.
template <typename I>
__device__ __forceinline__ I tap_index(int i, int W, int j) {   // pixel (i, j) of a W-wide sample
  if constexpr (sizeof(I) == sizeof(size_t) && !std::is_signed<I>::value) return (I)(i * W + j);
  else return (I)i * W + j;
}

// --------------------------------- max pool ------------------------------------
// nn.MaxPool2d(2): first maximum in (0,0),(0,1),(1,0),(1,1) order wins (strict >), as aten.
// window q with top-left pixel p00, channel quad c
template <typename I>
__device__ __forceinline__ void maxpool2_fwd_body(const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                  int ldo, I p00, I q, int W, int c) {
  const float4 a = ld4(x + p00 * ldx + c);
  const float4 b = ld4(x + (p00 + 1) * ldx + c);
  const float4 d = ld4(x + (p00 + W) * ldx + c);
  const float4 f = ld4(x + (p00 + W + 1) * ldx + c);
  st4(out + q * ldo + c, max2x2_first(a, b, d, f));
}

template <typename I>
__device__ __forceinline__ void maxpool2_bwd_body(const float* __restrict__ x, int ldx, const float* __restrict__ dout,
                                                  int lddo, float* __restrict__ dx, int lddx, I p0, I q, int W, int c,
                                                  int accumulate) {
  const I p[4] = {p0, p0 + 1, p0 + W, p0 + W + 1};
  float4 v[4], o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = ld4(x + p[k] * ldx + c);
  const float4 g = ld4(dout + q * lddo + c);
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = accumulate ? ld4(dx + p[k] * lddx + c) : zero4();
  route_argmax(v, g, o);
#pragma unroll
  for (int k = 0; k < 4; ++k) st4(dx + p[k] * lddx + c, o[k]);
}

__global__ void maxpool2_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, int N,
                                    int H, int W, int C) {
  const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
  const long long total = (long long)N * Ho * Wo * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C4) * 4;
    const long long q = e / C4;
    const int ox = (int)(q % Wo);
    const long long t = q / Wo;
    const int oy = (int)(t % Ho);
    const long long n = t / Ho;
    maxpool2_fwd_body<long long>(x, ldx, out, ldo, (n * H + 2 * oy) * W + 2 * ox, q, W, c);
  }
}

__global__ void maxpool2_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dout, int lddo,
                                    float* __restrict__ dx, int lddx, int N, int H, int W, int C, int accumulate) {
  const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
  const long long total = (long long)N * Ho * Wo * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C4) * 4;
    const long long q = e / C4;
    const int ox = (int)(q % Wo);
    const long long t = q / Wo;
    const int oy = (int)(t % Ho);
    const long long n = t / Ho;
    maxpool2_bwd_body<long long>(x, ldx, dout, lddo, dx, lddx, (n * H + 2 * oy) * W + 2 * ox, q, W, c, accumulate);
  }
}

// ----------------------------- bilinear upsample x2 ------------------------------
// output pixel (oy, ox) -> o; base: the sample's first pixel at the thread's channel quad
template <typename I>
__device__ __forceinline__ void upsample_fwd_body(const float* __restrict__ base, int ldx, float* __restrict__ o, int oy,
                                                  int ox, int H, int W, int Ho, int Wo) {
  const Lerp ly = lerp_index(oy, H, Ho), lx = lerp_index(ox, W, Wo);
  const float4 a = ld4(base + tap_index<I>(ly.i0, W, lx.i0) * ldx);
  const float4 b = ld4(base + tap_index<I>(ly.i0, W, lx.i1) * ldx);
  const float4 d = ld4(base + tap_index<I>(ly.i1, W, lx.i0) * ldx);
  const float4 f = ld4(base + tap_index<I>(ly.i1, W, lx.i1) * ldx);
  st4(o, bilerp4(ly, lx, a, b, d, f));
}

__global__ void upsample_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, int N,
                                    int H, int W, int Ho, int Wo, int C) {
  const int C4 = C >> 2;
  const long long total = (long long)N * Ho * Wo * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C4) * 4;
    const long long q = e / C4;
    const int ox = (int)(q % Wo);
    const long long t = q / Wo;
    const int oy = (int)(t % Ho);
    const long long n = t / Ho;
    upsample_fwd_body<long long>(x + n * H * W * (long long)ldx + c, ldx, out + q * ldo + c, oy, ox, H, W, Ho, Wo);
  }
}

// scalar-channel variant (any C): single-channel fields of PDEDataset / the cascade
__global__ void upsample_fwd_scalar_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo,
                                           int N, int H, int W, int Ho, int Wo, int C) {
  const long long total = (long long)N * Ho * Wo * C;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const long long q = e / C;
    const int ox = (int)(q % Wo);
    const long long t = q / Wo;
    const int oy = (int)(t % Ho);
    const long long n = t / Ho;
    const Lerp ly = lerp_index(oy, H, Ho), lx = lerp_index(ox, W, Wo);
    const float* base = x + n * H * W * (long long)ldx + c;
    const float a = base[((long long)ly.i0 * W + lx.i0) * ldx], b = base[((long long)ly.i0 * W + lx.i1) * ldx];
    const float d = base[((long long)ly.i1 * W + lx.i0) * ldx], f = base[((long long)ly.i1 * W + lx.i1) * ldx];
    out[q * ldo + c] = ly.l0 * (lx.l0 * a + lx.l1 * b) + ly.l1 * (lx.l0 * d + lx.l1 * f);
  }
}

// PDEDataset assembly (models.py:155-203) in one pass, one thread per fine pixel: the coarse
// field normalised with the FINE statistics tap by tap, then bilinearly resized to the fine grid
// (align_corners=True, the same lerp as upsample_fwd_scalar_kernel), theta normalised unless
// constant, f normalised, and the normalised target.  Each normalisation is (v - mean) / std with
// a correctly rounded division, as the reference's tensor expressions compute it.
// stats = {u_mean, u_std, f_mean, f_std, theta_mean, theta_std} (device, fp32).
__global__ __launch_bounds__(256) void pde_dataset_kernel(const float* __restrict__ uc, const float* __restrict__ uf,
                                                          const float* __restrict__ th, const float* __restrict__ fs,
                                                          const float* __restrict__ stats, int theta_const, int N,
                                                          int hc, int wc, int hf, int wf, float* __restrict__ inputs,
                                                          float* __restrict__ targets) {
  const long long plane = (long long)hf * wf, total = (long long)N * plane;
  const float um = stats[0], us = stats[1], fm = stats[2], fsd = stats[3], tm = stats[4], ts = stats[5];
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const long long n = q / plane;
    const int pix = (int)(q - n * plane), y = pix / wf, x = pix - y * wf;
    const Lerp ly = lerp_index(y, hc, hf), lx = lerp_index(x, wc, wf);
    const float* base = uc + n * hc * wc;
    const float a = (base[ly.i0 * wc + lx.i0] - um) / us, b = (base[ly.i0 * wc + lx.i1] - um) / us;
    const float d = (base[ly.i1 * wc + lx.i0] - um) / us, f = (base[ly.i1 * wc + lx.i1] - um) / us;
    float* in = inputs + n * 3 * plane + pix;
    in[0] = ly.l0 * (lx.l0 * a + lx.l1 * b) + ly.l1 * (lx.l0 * d + lx.l1 * f);
    in[plane] = theta_const ? th[q] : (th[q] - tm) / ts;
    in[2 * plane] = (fs[q] - fm) / fsd;
    targets[q] = (uf[q] - um) / us;
  }
}

// backward as a deterministic gather: every input pixel sums the output pixels whose
// 4-tap stencil touches it (scale < 1 => at most ~5 candidates per axis).
__device__ __forceinline__ int gather_weights(int i, int in, int out, int* idx, float* wt) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  int lo = 0, hi = out - 1;
  if (scale > 0.f) {
    lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
    hi = min(out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
  }
  int cnt = 0;
  for (int o = lo; o <= hi && cnt < 8; ++o) {
    const Lerp l = lerp_index(o, in, out);
    float w = 0.f;
    if (l.i0 == i) w += l.l0;
    if (l.i1 == i) w += l.l1;
    if (l.i0 == i || l.i1 == i) { idx[cnt] = o; wt[cnt] = w; ++cnt; }
  }
  return cnt;
}

// input pixel (iy, ix) -> o.  base: the sample's first output pixel at the thread's channel quad; sbase / wv: the
// sample's dsa and the quad's wg when the attention gating gradient dsa[q] * wg[c] joins dout (else null)
template <typename I>
__device__ __forceinline__ void upsample_bwd_body(const float* __restrict__ base, int lddo, float* __restrict__ o, int iy,
                                                  int ix, int H, int W, int Ho, int Wo, int accumulate,
                                                  const float* __restrict__ sbase, const float4& wv) {
  int oyi[8], oxi[8];
  float wy[8], wx[8];
  const int ny = gather_weights(iy, H, Ho, oyi, wy);
  const int nx = gather_weights(ix, W, Wo, oxi, wx);
  float4 s = zero4();
  for (int a = 0; a < ny; ++a) {
    float4 r = zero4();
    for (int b = 0; b < nx; ++b) {
      float4 g = ld4(base + tap_index<I>(oyi[a], Wo, oxi[b]) * lddo);
      if (sbase != nullptr) g = scale_add4(sbase[oyi[a] * Wo + oxi[b]], wv, g);
      r = fma4(r, wx[b], g);
    }
    s = fma4(s, wy[a], r);
  }
  if (accumulate) s = add4(s, ld4(o));
  st4(o, s);
}

__global__ void upsample_bwd_kernel(const float* __restrict__ dout, int lddo, float* __restrict__ dx, int lddx,
                                    int N, int H, int W, int Ho, int Wo, int C, int accumulate) {
  const int C4 = C >> 2;
  const long long total = (long long)N * H * W * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C4) * 4;
    const long long q = e / C4;
    const int ix = (int)(q % W);
    const long long t = q / W;
    const int iy = (int)(t % H);
    const long long n = t / H;
    upsample_bwd_body<long long>(dout + n * Ho * Wo * (long long)lddo + c, lddo, dx + q * lddx + c, iy, ix, H, W, Ho,
                                 Wo, accumulate, nullptr, zero4());
  }
}

// ---------------- pixel-blocked variants (C/4 a power of two <= 256) ----------------
// block = (C/4 channel quads) x (256 / (C/4) pixels): the channel quad is threadIdx.x and every
// thread derives its pixel once with 32-bit index math (the grid-stride kernels above divide a
// 64-bit element index per float4, which costs more than the memory access at these sizes).
__device__ __forceinline__ unsigned px_index() { return blockIdx.x * blockDim.y + threadIdx.y; }

__global__ __launch_bounds__(256) void maxpool2_fwd_px_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                              int ldo, unsigned npix, int H, int W) {
  const unsigned q = px_index();
  if (q >= npix) return;
  const unsigned Wo = W >> 1, Ho = H >> 1;
  const unsigned ox = q % Wo, t = q / Wo, oy = t % Ho, n = t / Ho;
  maxpool2_fwd_body<size_t>(x, ldx, out, ldo, ((size_t)n * H + 2 * oy) * W + 2 * ox, q, W, threadIdx.x * 4);
}

__global__ __launch_bounds__(256) void maxpool2_bwd_px_kernel(const float* __restrict__ x, int ldx,
                                                              const float* __restrict__ dout, int lddo,
                                                              float* __restrict__ dx, int lddx, unsigned npix, int H,
                                                              int W, int accumulate) {
  const unsigned q = px_index();
  if (q >= npix) return;
  const unsigned Wo = W >> 1, Ho = H >> 1;
  const unsigned ox = q % Wo, t = q / Wo, oy = t % Ho, n = t / Ho;
  maxpool2_bwd_body<size_t>(x, ldx, dout, lddo, dx, lddx, ((size_t)n * H + 2 * oy) * W + 2 * ox, q, W, threadIdx.x * 4,
                            accumulate);
}

__global__ __launch_bounds__(256) void upsample_fwd_px_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                              int ldo, unsigned npix, int H, int W, int Ho, int Wo) {
  const unsigned q = px_index();
  if (q >= npix) return;
  const unsigned ox = q % (unsigned)Wo, t = q / (unsigned)Wo, oy = t % (unsigned)Ho, n = t / (unsigned)Ho;
  const int c = threadIdx.x * 4;
  upsample_fwd_body<size_t>(x + (size_t)n * H * W * ldx + c, ldx, out + (size_t)q * ldo + c, oy, ox, H, W, Ho, Wo);
}

// upsample_fwd_px_kernel plus the spatial attention of the gate that reads the upsampled tensor
// (models.py:124-125: sa = sigmoid(conv1x1(g)) with g = up(d), models.py:89,92): the block's x
// threads hold one output pixel's channels, so the 1x1 conv is a shuffle reduction over them and g
// is not re-read for it.  c / 4 a power of two <= 64 (one pixel per half or whole wave).
// UPX pixel groups per block (blockDim.y pixels each), every group's four source loads issued before
// any interpolation: fewer, longer blocks with more loads in flight (the output write, 2/3 of the bytes,
// set the pace; 205 k eight-pixel blocks for u2 spent their time in dispatch and load latency)
constexpr int UPX = 4;
__global__ __launch_bounds__(256) void upsample_gate_fwd_px_kernel(const float* __restrict__ x, int ldx,
                                                                   float* __restrict__ out, int ldo, unsigned npix,
                                                                   int H, int W, int Ho, int Wo,
                                                                   const float* __restrict__ wg,
                                                                   const float* __restrict__ bg,
                                                                   float* __restrict__ sa) {
  const int c = threadIdx.x * 4;
  const float4 wv = ld4(wg + c);
  const float bias = bg[0];
  float4 a[UPX], b[UPX], d[UPX], f[UPX];
  Lerp ly[UPX], lx[UPX];
#pragma unroll
  for (int u = 0; u < UPX; ++u) {
    const unsigned q = (blockIdx.x * UPX + u) * blockDim.y + threadIdx.y;
    const unsigned qq = q < npix ? q : 0;
    const unsigned ox = qq % (unsigned)Wo, t = qq / (unsigned)Wo, oy = t % (unsigned)Ho, n = t / (unsigned)Ho;
    ly[u] = lerp_index(oy, H, Ho);
    lx[u] = lerp_index(ox, W, Wo);
    const float* base = x + (size_t)n * H * W * ldx + c;
    a[u] = ld4(base + (size_t)(ly[u].i0 * W + lx[u].i0) * ldx);
    b[u] = ld4(base + (size_t)(ly[u].i0 * W + lx[u].i1) * ldx);
    d[u] = ld4(base + (size_t)(ly[u].i1 * W + lx[u].i0) * ldx);
    f[u] = ld4(base + (size_t)(ly[u].i1 * W + lx[u].i1) * ldx);
  }
#pragma unroll
  for (int u = 0; u < UPX; ++u) {
    const unsigned q = (blockIdx.x * UPX + u) * blockDim.y + threadIdx.y;
    const bool on = q < npix;
    const float4 o = bilerp4(ly[u], lx[u], a[u], b[u], d[u], f[u]);
    if (on) st4(out + (size_t)q * ldo + c, o);
    float acc = dot4(o, wv);
    for (int off = 1; off < (int)blockDim.x; off <<= 1) acc += __shfl_xor(acc, off, 64);
    if (on && threadIdx.x == 0) sa[q] = 1.f / (1.f + expf(-(acc + bias)));
  }
}

// The spatial attention of a gate whose gating input is up(x), from x at low resolution: the 1x1 conv
// commutes with the bilinear upsample, sa = sigmoid(up(x . wg) + bg) (models.py:124-125 with
// g = up(d), :89 / :92) -- for a decoder conv that reads up(x) without materialising it.  The dot
// products reduce like upsample_gate_fwd_px_kernel's (one pixel per c/4 threads, shuffle tree).
__global__ __launch_bounds__(256) void gate_dot_px_kernel(const float* __restrict__ x, int ldx, unsigned npix,
                                                          const float* __restrict__ wg, float* __restrict__ t) {
  const unsigned q = px_index();
  const bool on = q < npix;
  const int c = threadIdx.x * 4;
  const float4 wv = ld4(wg + c);
  const float4 o = on ? ld4(x + (size_t)q * ldx + c) : zero4();
  float acc = dot4(o, wv);
  for (int off = 1; off < (int)blockDim.x; off <<= 1) acc += __shfl_xor(acc, off, 64);
  if (on && threadIdx.x == 0) t[q] = acc;
}

__global__ __launch_bounds__(256) void up_sigmoid_kernel(const float* __restrict__ t, float* __restrict__ sa,
                                                         unsigned npix, int H, int W, int Ho, int Wo,
                                                         const float* __restrict__ bg) {
  const unsigned q = blockIdx.x * 256 + threadIdx.x;
  if (q >= npix) return;
  const unsigned ox = q % (unsigned)Wo, r = q / (unsigned)Wo, oy = r % (unsigned)Ho, n = r / (unsigned)Ho;
  const Lerp ly = lerp_index(oy, H, Ho), lx = lerp_index(ox, W, Wo);
  const float* b = t + (size_t)n * H * W;
  const float a0 = b[ly.i0 * W + lx.i0], a1 = b[ly.i0 * W + lx.i1], d0 = b[ly.i1 * W + lx.i0], d1 = b[ly.i1 * W + lx.i1];
  const float v = ly.l0 * (lx.l0 * a0 + lx.l1 * a1) + ly.l1 * (lx.l0 * d0 + lx.l1 * d1);
  sa[q] = 1.f / (1.f + expf(-(v + bg[0])));
}

// gsa / gw (nullable): the attention gating gradient folded in, the upsampled tensor's gradient
// being dout[q][c] + gsa[q] * gw[c] (srpde_upsample_bilinear_bwd_gated)
__global__ __launch_bounds__(256) void upsample_bwd_px_kernel(const float* __restrict__ dout, int lddo,
                                                              float* __restrict__ dx, int lddx, unsigned npix, int H,
                                                              int W, int Ho, int Wo, int accumulate,
                                                              const float* __restrict__ gsa = nullptr,
                                                              const float* __restrict__ gw = nullptr) {
  const unsigned q = px_index();
  if (q >= npix) return;
  const unsigned ix = q % (unsigned)W, t = q / (unsigned)W, iy = t % (unsigned)H, n = t / (unsigned)H;
  const int c = threadIdx.x * 4;
  const float4 wv = gw != nullptr ? ld4(gw + c) : zero4();
  const float* sbase = gsa != nullptr ? gsa + (size_t)n * Ho * Wo : nullptr;
  upsample_bwd_body<size_t>(dout + (size_t)n * Ho * Wo * lddo + c, lddo, dx + (size_t)q * lddx + c, iy, ix, H, W, Ho, Wo,
                            accumulate, sbase, wv);
}

// Row-blocked upsample backward: one workgroup per (sample, input row iy), all channels.  Phase 1
// reduces iy's candidate output rows with their y weights (and the attention gating gradient,
// GATED) into an LDS row R[ox][c]: every gradient element is read once per workgroup, the
// candidate rows' loads of a thread independent of each other.  Phase 2 applies the x weights
// from LDS.  Needs at most ROWS_NS candidate rows (upsample_rows_ok) and C/4 dividing 256.
// The pixel-blocked gather above re-read each gradient element ~4x through L2 with one load per
// trip (2.35 TB/s isolated).
constexpr int ROWS_NS = 6;
// bijective block remap: XCD x (= bid % 8 in dispatch order) takes the x-th contiguous eighth
__device__ __forceinline__ int xcd_rows_remap(int bid, int total) {
  const int xcd = bid & 7, q = total >> 3, r = total & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}
// weight of output o in input i's gradient (gather_weights' per-candidate term); the candidates of
// i form one contiguous range of o (i0 and i1 are monotone in o)
__device__ __forceinline__ float cand_weight(int o, int i, int in, int out, bool* hit) {
  const Lerp l = lerp_index(o, in, out);
  *hit = l.i0 == i || l.i1 == i;
  return (l.i0 == i ? l.l0 : 0.f) + (l.i1 == i ? l.l1 : 0.f);
}
__device__ __forceinline__ void cand_range(int i, int in, int out, int* lo, int* hi) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  *lo = 0;
  *hi = out - 1;
  if (scale > 0.f) {
    *lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
    *hi = min(out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
  }
}

// phase 1 of upsample_bwd_rows_kernel with NSL candidate-row slots (slots past the range re-read
// the first row, branch-free, with weight 0)
template <bool GATED, int NSL>
__device__ __forceinline__ void upsample_rows_phase1(const float* __restrict__ dout, int lddo, int Ho, int Wo, int C4,
                                                     int n, int iy, int H, int oy0, int hi,
                                                     const float* __restrict__ gsa, const float* __restrict__ gw,
                                                     float4* rrow) {
  const int cq = threadIdx.x % C4, lx0 = threadIdx.x / C4, nlx = blockDim.x / C4;
  float wy[NSL];
#pragma unroll
  for (int a = 0; a < NSL; ++a) {
    bool hit = false;
    const float w = oy0 + a <= hi ? cand_weight(oy0 + a, iy, H, Ho, &hit) : 0.f;
    wy[a] = hit ? w : 0.f;
  }
  const float4 wv = GATED ? ld4(gw + cq * 4) : zero4();
  const float* base = dout + (size_t)n * Ho * Wo * lddo + cq * 4;
  const float* sb = GATED ? gsa + (size_t)n * Ho * Wo : nullptr;
  for (int ox = lx0; ox < Wo; ox += nlx) {
    float4 g[NSL];
    float sv[NSL];
#pragma unroll
    for (int a = 0; a < NSL; ++a) {
      const int o = (oy0 + a <= hi ? oy0 + a : oy0) * Wo + ox;
      g[a] = ld4(base + (size_t)o * lddo);
      if constexpr (GATED) sv[a] = sb[o];
    }
    float4 r = zero4();
#pragma unroll
    for (int a = 0; a < NSL; ++a) {   // zero-weight slots add nothing (0 * finite)
      float4 gg = g[a];
      if constexpr (GATED) gg = scale_add4(sv[a], wv, gg);
      r = fma4(r, wy[a], gg);
    }
    rrow[ox * C4 + cq] = r;
  }
}

// The BatchNorm (+ ReLU) whose output gradient the upsample backward writes (the decoder block below:
// dec2.bn2 under u2, dec3.bn2 under u3): its backward reduction is formed from the values as they are
// stored, so the BN backward does not re-read them (bn_bwd_reduce_kernel's expressions; partials per
// input row block: part[row][C] = (sum dz, sum dz * xhat), da_max[row] = max |dx|)
struct UpBnArgs {
  const float* y;
  int ldy;
  const float *mean, *invstd, *gamma, *beta;
  int relu;
  float2* part;
  float* da_max;
};

template <bool GATED, bool BN = false>
__global__ __launch_bounds__(256) void upsample_bwd_rows_kernel(const float* __restrict__ dout, int lddo,
                                                                float* __restrict__ dx, int lddx, int H, int W, int Ho,
                                                                int Wo, int C, int accumulate,
                                                                const float* __restrict__ gsa,
                                                                const float* __restrict__ gw, UpBnArgs bn = {}) {
  extern __shared__ float4 rrow[];   // [Wo][C/4]; with BN at least [2][256] for the block reduction
  const int C4 = C >> 2;
  const int cq = threadIdx.x % C4, lx0 = threadIdx.x / C4, nlx = blockDim.x / C4;
  // consecutive workgroups go to different XCDs (each with its own L2): remap so an XCD walks a
  // contiguous run of rows and the output rows two neighbouring input rows share hit its L2
  const int blk = xcd_rows_remap(blockIdx.x, gridDim.x);
  const int n = blk / H, iy = blk - n * H;
  // iy's candidate output rows: [oy0, last], contiguous, at most ROWS_NS (upsample_rows_ok)
  int lo, hi;
  cand_range(iy, H, Ho, &lo, &hi);
  int oy0 = hi + 1;
  for (int o = lo; o <= hi && oy0 > hi; ++o) {
    bool hit;
    cand_weight(o, iy, H, Ho, &hit);
    if (hit) oy0 = o;
  }
  if (oy0 > hi) oy0 = lo;   // no candidate (not reached for valid shapes): all weights 0, loads in range
  int last = oy0;
  for (int o = oy0 + 1; o <= hi && o < oy0 + ROWS_NS; ++o) {
    bool hit;
    cand_weight(o, iy, H, Ho, &hit);
    if (hit) last = o;
  }
  // the row count is uniform over the workgroup: one instantiation per count, no wasted loads
  const int nrow = last - oy0 + 1;
  if (nrow <= 3) upsample_rows_phase1<GATED, 3>(dout, lddo, Ho, Wo, C4, n, iy, H, oy0, hi, gsa, gw, rrow);
  else if (nrow == 4) upsample_rows_phase1<GATED, 4>(dout, lddo, Ho, Wo, C4, n, iy, H, oy0, hi, gsa, gw, rrow);
  else if (nrow == 5) upsample_rows_phase1<GATED, 5>(dout, lddo, Ho, Wo, C4, n, iy, H, oy0, hi, gsa, gw, rrow);
  else upsample_rows_phase1<GATED, ROWS_NS>(dout, lddo, Ho, Wo, C4, n, iy, H, oy0, hi, gsa, gw, rrow);
  __syncthreads();
  BnBwdAcc acc;
  if constexpr (BN) acc.load(bn.mean, bn.invstd, bn.gamma, bn.beta, cq * 4);
  for (int ix = lx0; ix < W; ix += nlx) {
    int xlo, xhi;
    cand_range(ix, W, Wo, &xlo, &xhi);
    float4 s = zero4();
    for (int o = xlo; o <= xhi; ++o) {
      bool hit;
      const float w = cand_weight(o, ix, W, Wo, &hit);
      if (hit) s = fma4(s, w, rrow[o * C4 + cq]);
    }
    float* o = dx + ((size_t)blk * W + ix) * lddx + cq * 4;
    if (accumulate) s = add4(s, ld4(o));
    st4(o, s);
    if constexpr (BN) {
      const float4 v = ld4(bn.y + ((size_t)blk * W + ix) * bn.ldy + cq * 4);
      acc.amax(s);
      acc.add(v, s, bn.relu);
    }
  }
  if constexpr (BN) {
    // bn_bwd_block_combine's steps around this kernel's own LDS use: the sums go where the row was (only the
    // threads that own a slot write), the waves' maxima behind them, so one barrier serves both
    __syncthreads();   // every thread is past its rrow reads
    const int t = threadIdx.x;
    if (lx0 < nlx) {
      rrow[t] = acc.s1;
      rrow[256 + t] = acc.s2;
    }
    const float dmax = wave_max(acc.dmax);
    float* wmx = reinterpret_cast<float*>(rrow + 512);
    if ((t & 63) == 0) wmx[t >> 6] = dmax;
    __syncthreads();
    if (t < C4) bn_bwd_store_part(rrow, C4, nlx, t, bn.part + (size_t)blk * C + t * 4);
    if (t == 0) bn.da_max[blk] = max4slots(wmx);
  }
}

// the gather's cap of 8 candidates per axis (gather_weights) holds for scale = (in-1)/(out-1) > 1/4:
// input i's candidates are the outputs o with floor(o * scale) in {i-1, i}, at most
// floor(2 / scale) + 1 of them
static bool upsample_gather_ok(int in, int out) { return out <= 1 || in <= 1 || 2.0 * (out - 1) < 8.0 * (in - 1); }

// the row-blocked kernel: input row i's candidate rows number at most floor(2/scale) + 1 (+1 for
// rounding) <= ROWS_NS when 2/scale < 5; C/4 a power of two <= 256; one LDS row of Wo x C floats
static bool upsample_rows_ok(int h, int w, int ho, int wo, int c, int lddo, int lddx) {
  const int c4 = c / 4;
  return c % 4 == 0 && c4 >= 1 && c4 <= 256 && (c4 & (c4 - 1)) == 0 && lddo % 4 == 0 && lddx % 4 == 0 &&
         h > 1 && ho > 1 && 2.0 * (ho - 1) < 5.0 * (h - 1) && upsample_gather_ok(w, wo) &&
         (size_t)wo * c * sizeof(float) <= 64 * 1024;
}

template <bool GATED>
static void launch_upsample_bwd_rows(const float* dout, int lddo, float* dx, int lddx, int n, int h, int w, int ho,
                                     int wo, int c, int accumulate, const float* gsa, const float* gw,
                                     hipStream_t stream, const UpBnArgs* bn = nullptr) {
  if (bn != nullptr) {
    const size_t lds = std::max((size_t)wo * c * sizeof(float), (size_t)(512 * sizeof(float4) + 16));
    hipLaunchKernelGGL((upsample_bwd_rows_kernel<GATED, true>), dim3((unsigned)(n * h)), dim3(256), lds, stream, dout,
                       lddo, dx, lddx, h, w, ho, wo, c, accumulate, gsa, gw, *bn);
    return;
  }
  hipLaunchKernelGGL((upsample_bwd_rows_kernel<GATED, false>), dim3((unsigned)(n * h)), dim3(256),
                     (size_t)wo * c * sizeof(float), stream, dout, lddo, dx, lddx, h, w, ho, wo, c, accumulate, gsa, gw,
                     UpBnArgs{});
}

static int grid_for(long long total, int cap = 8192) {
  long long b = (total + 255) / 256;
  if (b < 1) b = 1;
  return (int)std::min<long long>(b, cap);
}

// launch geometry of the pixel-blocked kernels, or false when C/4 is not a power of two <= 256
static bool px_geometry(long long npix, int c, dim3* grid, dim3* block) {
  const int c4 = c / 4;
  if (c % 4 != 0 || c4 < 1 || c4 > 256 || (c4 & (c4 - 1)) != 0 || npix >= (1LL << 31)) return false;
  const int py = 256 / c4;
  *block = dim3(c4, py);
  *grid = dim3((unsigned)((npix + py - 1) / py));
  return true;
}

// the pixel-blocked kernel of a pair where px_geometry takes the shape (px(grid, block, npix)), else the
// grid-stride kernel over the npix * c / 4 quads (gs(grid))
template <typename PX, typename GS>
static void launch_px_or_grid_stride(long long npix, int c, PX&& px, GS&& gs) {
  dim3 g, b;
  if (px_geometry(npix, c, &g, &b)) px(g, b, (unsigned)npix);
  else gs(dim3(grid_for(npix * (c / 4))));
}

// ------------------------------- attention gate ----------------------------------
// channel branch: m = mean_hw(x); h = relu(W1 m + b1); ca = sigmoid(W2 h + b2)  (models.py:106-112)
// one block per sample
__global__ __launch_bounds__(256) void att_channel_fwd_kernel(const float* __restrict__ x, int ldx, int HW, int C,
                                                              int Cr, const float* __restrict__ w1,
                                                              const float* __restrict__ b1,
                                                              const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ m,
                                                              float* __restrict__ h, float* __restrict__ ca) {
  extern __shared__ float sh[];  // [256*4] partials, then m[C], h[Cr]
  const int n = blockIdx.x, C4 = C >> 2;
  const int c4 = threadIdx.x % C4, r0 = threadIdx.x / C4, rs = blockDim.x / C4;
  const int active = C4 * rs;
  float4 s = zero4();
  if ((int)threadIdx.x < active) {
    const float* base = x + (long long)n * HW * ldx + c4 * 4;
    for (int p = r0; p < HW; p += rs) {
      const float4 v = ld4(base + (long long)p * ldx);
      s = add4(s, v);
    }
  }
  float4* red = reinterpret_cast<float4*>(sh);
  red[threadIdx.x] = s;
  __syncthreads();
  float* ms = sh + 4 * 256;
  float* hs = ms + C;
  if ((int)threadIdx.x < C4) {
    const float4 t = rowsum4(red, C4, rs, threadIdx.x);
    const float inv = 1.f / (float)HW;
    const int c = threadIdx.x * 4;
    ms[c] = t.x * inv; ms[c + 1] = t.y * inv; ms[c + 2] = t.z * inv; ms[c + 3] = t.w * inv;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < C; j += blockDim.x) m[(long long)n * C + j] = ms[j];
  for (int r = threadIdx.x; r < Cr; r += blockDim.x) {
    float a = b1[r];
    for (int c = 0; c < C; ++c) a += w1[r * C + c] * ms[c];
    a = fmaxf(a, 0.f);
    hs[r] = a;
    h[(long long)n * Cr + r] = a;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = b2[c];
    for (int r = 0; r < Cr; ++r) a += w2[c * Cr + r] * hs[r];
    ca[(long long)n * C + c] = 1.f / (1.f + expf(-a));
  }
}

// spatial branch: sa[p] = sigmoid(sum_c g[p][c] wg[c] + bg), 8 lanes per pixel  (models.py:114-117)
__global__ __launch_bounds__(256) void att_spatial_fwd_kernel(const float* __restrict__ g, int ldg, long long P,
                                                              int G, const float* __restrict__ wg,
                                                              const float* __restrict__ bg, float* __restrict__ sa) {
  const int sub = threadIdx.x & 7;
  for (long long p = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 3; p < P;
       p += ((long long)gridDim.x * blockDim.x) >> 3) {
    float acc = 0.f;
    const float* row = g + p * ldg;
    for (int c = sub * 4; c < G; c += 32) {
      const float4 v = ld4(row + c);
      const float4 w = ld4(wg + c);
      acc += dot4(v, w);
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (sub == 0) sa[p] = 1.f / (1.f + expf(-(acc + bg[0])));
  }
}

// out[p][c] = (x[p][c] * ca[n][c]) * sa[p]   (models.py:122, :128)
__global__ void att_apply_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ ca,
                                 const float* __restrict__ sa, float* __restrict__ out, int ldo, long long P, int HW,
                                 int C) {
  const int C4 = C >> 2;
  const long long total = P * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long p = e / C4;
    const int c = (int)(e - p * C4) * 4;
    const long long n = p / HW;
    const float4 v = ld4(x + p * ldx + c);
    const float4 a = ld4(ca + n * C + c);
    const float s = sa[p];
    float4 o;
    o.x = (v.x * a.x) * s; o.y = (v.y * a.y) * s; o.z = (v.z * a.z) * s; o.w = (v.w * a.w) * s;
    *reinterpret_cast<float4*>(out + p * ldo + c) = o;
  }
}

// backward, pass 1 (per pixel): dsa_pre[p] = sigmoid'(sa) * sum_c dout * (x * ca)
__global__ __launch_bounds__(256) void att_bwd_pixel_kernel(const float* __restrict__ dout, int lddo,
                                                            const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ ca,
                                                            const float* __restrict__ sa, long long P, int HW, int C,
                                                            float* __restrict__ dsa_pre) {
  const int sub = threadIdx.x & 7;
  for (long long p = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 3; p < P;
       p += ((long long)gridDim.x * blockDim.x) >> 3) {
    const long long n = p / HW;
    float acc = 0.f;
    for (int c = sub * 4; c < C; c += 32) {
      const float4 d = ld4(dout + p * lddo + c);
      const float4 v = ld4(x + p * ldx + c);
      const float4 a = ld4(ca + n * C + c);
      acc += d.x * (v.x * a.x) + d.y * (v.y * a.y) + d.z * (v.z * a.z) + d.w * (v.w * a.w);
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (sub == 0) {
      const float s = sa[p];
      dsa_pre[p] = acc * (1.f - s) * s;
    }
  }
}

// backward, pass 2 (one block per sample): dca[c] = sum_hw dout*sa*x; MLP backward;
// writes dm[n][c] (grad of the spatial mean) and per-sample weight-grad rows.
__global__ __launch_bounds__(256) void att_bwd_channel_kernel(
    const float* __restrict__ dout, int lddo, const float* __restrict__ x, int ldx, const float* __restrict__ sa,
    int HW, int C, int Cr, const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ m,
    const float* __restrict__ h, const float* __restrict__ ca, float* __restrict__ dm,
    float* __restrict__ dw1_rows, float* __restrict__ db1_rows, float* __restrict__ dw2_rows,
    float* __restrict__ db2_rows) {
  extern __shared__ float sh[];
  const int n = blockIdx.x, C4 = C >> 2;
  const int c4 = threadIdx.x % C4, r0 = threadIdx.x / C4, rs = blockDim.x / C4;
  const int active = C4 * rs;
  float4 s = zero4();
  if ((int)threadIdx.x < active) {
    const long long pb = (long long)n * HW;
    for (int p = r0; p < HW; p += rs) {
      const float4 d = ld4(dout + (pb + p) * lddo + c4 * 4);
      const float4 v = ld4(x + (pb + p) * ldx + c4 * 4);
      const float q = sa[pb + p];
      s.x += (d.x * q) * v.x; s.y += (d.y * q) * v.y; s.z += (d.z * q) * v.z; s.w += (d.w * q) * v.w;
    }
  }
  float4* red = reinterpret_cast<float4*>(sh);
  red[threadIdx.x] = s;
  __syncthreads();
  float* dpre = sh + 4 * 256;  // [C] grad of pre-sigmoid channel logits
  float* dh = dpre + C;        // [Cr]
  if ((int)threadIdx.x < C4) {
    const float4 t = rowsum4(red, C4, rs, threadIdx.x);
    const int c = threadIdx.x * 4;
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = ca[(long long)n * C + c + k];
      dpre[c + k] = tv[k] * (1.f - a) * a;
    }
  }
  __syncthreads();
  // per-sample vectors only; the weight grads are batch reductions (outer_sum_kernel)
  for (int c = threadIdx.x; c < C; c += blockDim.x) db2_rows[(long long)n * C + c] = dpre[c];
  for (int r = threadIdx.x; r < Cr; r += blockDim.x) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += w2[c * Cr + r] * dpre[c];
    a = h[(long long)n * Cr + r] > 0.f ? a : 0.f;
    dh[r] = a;
    db1_rows[(long long)n * Cr + r] = a;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = 0.f;
    for (int r = 0; r < Cr; ++r) a += w1[r * C + c] * dh[r];
    dm[(long long)n * C + c] = a / (float)HW;
  }
}

// backward, passes 1 and 2 in one read of dout and x (one block per sample, C / 4 in {16, 32, 64}):
// dsa_pre[p] = sigmoid'(sa) * sum_c dout * (x * ca)   (the C / 4 lanes of a pixel reduce by shuffles)
// and dca[c] = sum_hw dout * sa * x, then the channel-MLP backward exactly as att_bwd_channel_kernel.
__global__ __launch_bounds__(256) void att_bwd_sample_kernel(
    const float* __restrict__ dout, int lddo, const float* __restrict__ x, int ldx, const float* __restrict__ sa,
    int HW, int C, int Cr, const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ m,
    const float* __restrict__ h, const float* __restrict__ ca, float* __restrict__ dm, float* __restrict__ dw1_rows,
    float* __restrict__ db1_rows, float* __restrict__ dw2_rows, float* __restrict__ db2_rows,
    float* __restrict__ dsa_pre) {
  extern __shared__ float sh[];
  const int n = blockIdx.x, C4 = C >> 2;
  const int c4 = threadIdx.x % C4, r0 = threadIdx.x / C4, rs = blockDim.x / C4;
  float4 s = zero4();
  {
    const float4 a = ld4(ca + (long long)n * C + c4 * 4);
    const long long pb = (long long)n * HW;
    for (int p = r0; p < HW; p += rs) {   // every lane of a pixel's C / 4 group takes the same trips
      const float4 d = ld4(dout + (pb + p) * lddo + c4 * 4);
      const float4 v = ld4(x + (pb + p) * ldx + c4 * 4);
      const float q = sa[pb + p];
      s.x += (d.x * q) * v.x; s.y += (d.y * q) * v.y; s.z += (d.z * q) * v.z; s.w += (d.w * q) * v.w;
      float dot = d.x * (v.x * a.x) + d.y * (v.y * a.y) + d.z * (v.z * a.z) + d.w * (v.w * a.w);
      for (int o = C4 >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
      if (c4 == 0) dsa_pre[pb + p] = dot * (1.f - q) * q;
    }
  }
  float4* red = reinterpret_cast<float4*>(sh);
  red[threadIdx.x] = s;
  __syncthreads();
  float* dpre = sh + 4 * 256;  // [C] grad of pre-sigmoid channel logits
  float* dh = dpre + C;        // [Cr]
  if ((int)threadIdx.x < C4) {
    const float4 t = rowsum4(red, C4, rs, threadIdx.x);
    const int c = threadIdx.x * 4;
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = ca[(long long)n * C + c + k];
      dpre[c + k] = tv[k] * (1.f - a) * a;
    }
  }
  __syncthreads();
  // per-sample vectors only; the weight grads are batch reductions (outer_sum_kernel)
  for (int c = threadIdx.x; c < C; c += blockDim.x) db2_rows[(long long)n * C + c] = dpre[c];
  for (int r = threadIdx.x; r < Cr; r += blockDim.x) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += w2[c * Cr + r] * dpre[c];
    a = h[(long long)n * Cr + r] > 0.f ? a : 0.f;
    dh[r] = a;
    db1_rows[(long long)n * Cr + r] = a;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = 0.f;
    for (int r = 0; r < Cr; ++r) a += w1[r * C + c] * dh[r];
    dm[(long long)n * C + c] = a / (float)HW;
  }
}

// backward, pass 3 (elementwise): dx = (dout*sa)*ca + dm[n][c]  (write or accumulate)
__global__ void att_bwd_dx_kernel(const float* __restrict__ dout, int lddo, const float* __restrict__ ca,
                                  const float* __restrict__ sa, const float* __restrict__ dm, float* __restrict__ dx,
                                  int lddx, long long P, int HW, int C, int accumulate) {
  const int C4 = C >> 2;
  const long long total = P * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long p = e / C4;
    const int c = (int)(e - p * C4) * 4;
    const long long n = p / HW;
    const float4 d = ld4(dout + p * lddo + c);
    const float4 a = ld4(ca + n * C + c);
    const float4 g = ld4(dm + n * C + c);
    const float s = sa[p];
    float4 o = gate_dx4(d, s, a, g);
    float* dst = dx + p * lddx + c;
    if (accumulate) o = add4(o, ld4(dst));
    st4(dst, o);
  }
}

// backward, gating: dg[p][c] (+)= dsa_pre[p] * wg[c]
__global__ void att_bwd_gating_kernel(const float* __restrict__ dsa_pre, const float* __restrict__ wg,
                                      float* __restrict__ dg, int lddg, long long P, int G, int accumulate) {
  const int G4 = G >> 2;
  const long long total = P * G4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long p = e / G4;
    const int c = (int)(e - p * G4) * 4;
    const float s = dsa_pre[p];
    const float4 w = ld4(wg + c);
    float4 o = scale4(s, w);
    float* dst = dg + p * lddg + c;
    if (accumulate) o = add4(o, ld4(dst));
    st4(dst, o);
  }
}

// column partial sums of v[p][c]*s[p] over a row block, plus sum s[p] in column C (float2 .x).
// Used for the spatial-gate weight grad (v = gating, s = dsa_pre) and for the head (v = z, s = dout).
__global__ __launch_bounds__(256) void weighted_colsum_kernel(const float* __restrict__ v, int ldv,
                                                              const float* __restrict__ s, long long P, int C,
                                                              int rows_per_blk, float2* __restrict__ part) {
  extern __shared__ float4 red4[];
  const int C4 = C >> 2;
  const int c4 = threadIdx.x % C4, r0 = threadIdx.x / C4, rs = blockDim.x / C4;
  const int active = C4 * rs;
  float4 acc = zero4();
  float sacc = 0.f;
  const long long pb = (long long)blockIdx.x * rows_per_blk;
  const long long pe = min(P, pb + rows_per_blk);
  if ((int)threadIdx.x < active) {
    auto row = [&](const float4& a, float w) {
      acc.x += a.x * w; acc.y += a.y * w; acc.z += a.z * w; acc.w += a.w * w;
      if (c4 == 0) sacc += w;
    };
    long long p = pb + r0;
    for (; p + 3 * rs < pe; p += 4 * rs) {   // four rows' loads before their in-order sums
      float4 a[4];
      float w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = ld4(v + (p + u * rs) * ldv + c4 * 4);
        w[u] = s[p + u * rs];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) row(a[u], w[u]);
    }
    for (; p < pe; p += rs) row(ld4(v + p * ldv + c4 * 4), s[p]);
  }
  red4[threadIdx.x] = acc;
  red4[256 + threadIdx.x] = make_float4(sacc, 0.f, 0.f, 0.f);
  __syncthreads();
  if ((int)threadIdx.x < C4) {
    float4 t = zero4();
    float ts = 0.f;
    for (int r = 0; r < rs; ++r) {
      const float4 a = red4[r * C4 + threadIdx.x];
      t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w;
      if (threadIdx.x == 0) ts += red4[256 + r * C4].x;
    }
    float2* o = part + (size_t)blockIdx.x * (C + 1);
    const int c = threadIdx.x * 4;
    o[c] = make_float2(t.x, 0.f); o[c + 1] = make_float2(t.y, 0.f);
    o[c + 2] = make_float2(t.z, 0.f); o[c + 3] = make_float2(t.w, 0.f);
    if (threadIdx.x == 0) o[C] = make_float2(ts, 0.f);
  }
}

// out[i][j] = sum_n a[n][i] * b[n][j]  (a or b null => 1): the 1x1 channel-MLP weight and
// bias grads as batch reductions.  grid (la, ceil(lb/64)), 1024 threads = 64 j-lanes x 16
// sample groups, fp64 partials combined in fixed order (deterministic).
__global__ __launch_bounds__(1024) void outer_sum_kernel(const float* __restrict__ a, int la,
                                                         const float* __restrict__ b, int lb, int n,
                                                         float* __restrict__ out) {
  __shared__ double red[16][64];
  const int i = blockIdx.x, jl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int j = blockIdx.y * 64 + jl;
  double s = 0.0;
  if (j < lb) {
    int k = grp;
    for (; k + 7 * 16 < n; k += 8 * 16) {   // eight samples' loads before their in-order products
      float av[8], bv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        av[u] = a ? a[(long long)(k + 16 * u) * la + i] : 1.f;
        bv[u] = b ? b[(long long)(k + 16 * u) * lb + j] : 1.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (double)av[u] * (double)bv[u];
    }
    for (; k < n; k += 16) {
      const double av = a ? (double)a[(long long)k * la + i] : 1.0;
      const double bv = b ? (double)b[(long long)k * lb + j] : 1.0;
      s += av * bv;
    }
  }
  red[grp][jl] = s;
  __syncthreads();
  if (grp == 0 && j < lb) {
    double t = 0.0;
    for (int g = 0; g < 16; ++g) t += red[g][jl];
    out[(long long)i * lb + j] = (float)t;
  }
}

// fixed-order fp64 sum of rows [n][len] -> out[len]  (per-sample bias-grad rows)
__global__ void rowsum_kernel(const float* __restrict__ rows, int n, int len, float* __restrict__ out, int stride_in,
                              int accumulate) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= len) return;
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += rows[(long long)k * stride_in + j];
  out[j] = accumulate ? out[j] + (float)s : (float)s;
}

// fp64 sums over blocks of float2 partials [nblk][len] (.x) -> out[len]
__global__ void partsum_kernel(const float2* __restrict__ part, int nblk, int len, float* __restrict__ out) {
  const int j = blockIdx.x;
  __shared__ double a[256];
  double s = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) s += part[(size_t)k * len + j].x;
  a[threadIdx.x] = s;
  __syncthreads();
  for (int t = 128; t > 0; t >>= 1) {
    if ((int)threadIdx.x < t) a[threadIdx.x] += a[threadIdx.x + t];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[j] = (float)a[0];
}

// -------------------------------- output head ------------------------------------
// out[p] = (bf + sum_c z[p][c] wf[c]) + x_in[n][0][p]   (final 1x1 conv + residual)
__global__ void head_fwd_kernel(const float* __restrict__ z, int ldz, int C, const float* __restrict__ wf,
                                const float* __restrict__ bf, const float* __restrict__ xin, int xin_c, int HW,
                                long long P, float* __restrict__ out) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int c = 0; c < C; c += 4) {
      const float4 v = ld4(z + p * ldz + c);
      acc += v.x * wf[c] + v.y * wf[c + 1] + v.z * wf[c + 2] + v.w * wf[c + 3];
    }
    const long long n = p / HW;
    const int q = (int)(p - n * HW);
    out[p] = (acc + bf[0]) + xin[(n * xin_c) * HW + q];
  }
}

// dz[p][c] = dout[p] * wf[c]
__global__ void head_bwd_dz_kernel(const float* __restrict__ dout, const float* __restrict__ wf, int C,
                                   float* __restrict__ dz, int lddz, long long P) {
  const int C4 = C >> 2;
  const long long total = P * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long p = e / C4;
    const int c = (int)(e - p * C4) * 4;
    const float d = dout[p];
    *reinterpret_cast<float4*>(dz + p * lddz + c) = make_float4(d * wf[c], d * wf[c + 1], d * wf[c + 2], d * wf[c + 3]);
  }
}

// ----------------------------------- MSE ------------------------------------------
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                          long long n, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float d = y[i] - t[i];
    s += (double)(d * d);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void mse_final_kernel(const double* __restrict__ part, int nblk, long long n, float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) s += part[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)n);
}

// dy = 2 (y - t) / n * gout
__global__ void mse_bwd_kernel(const float* __restrict__ y, const float* __restrict__ t, long long n,
                               const float* __restrict__ gout, float* __restrict__ dy) {
  const float g = gout ? gout[0] : 1.f;
  const float norm = 2.f / (float)n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dy[i] = norm * (y[i] - t[i]) * g;
}

// the channel counts weighted_colsum_kernel (and so colsum_blocks) takes: 1..256 float4 lanes per row
static bool colsum_ok(int C) { return C % 4 == 0 && C >= 4 && C <= 1024; }
// ... and the per-sample attention kernels' c (att_lds_bytes, cr = c / 8) beside the gating input's gc
static bool att_bwd_counts_ok(int c, int gc) { return c % 32 == 0 && c >= 32 && c <= 1024 && colsum_ok(gc); }

static int colsum_blocks(long long P, int C, int* rpb) {
  const int rs = 256 / (C >> 2);
  long long r = (P + 1023) / 1024;
  r = (r + rs - 1) / rs * rs;
  if (r < rs) r = rs;
  *rpb = (int)r;
  return (int)((P + r - 1) / r);
}

}  // namespace srpde

using namespace srpde;

extern "C" {

int srpde_nchw_to_nhwc(const float* x, float* out, int n, int cin, int h, int w, int cpad, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && out && cpad >= cin, "srpde_nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for((long long)n * h * w)), dim3(256), 0, stream, x, out, n, cin,
                     h * w, cpad);
  SRPDE_LAUNCH_CHECK("srpde_nchw_to_nhwc");
  return 0;
}

int srpde_nhwc_to_nchw(const float* x, int ldx, float* out, int n, int c, int h, int w, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && out && n > 0 && c > 0 && ldx >= c, "srpde_nhwc_to_nchw: bad args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((long long)n * c * h * w)), dim3(256), 0, stream, x, ldx, out,
                     n, c, h * w);
  SRPDE_LAUNCH_CHECK("srpde_nhwc_to_nchw");
  return 0;
}

int srpde_axpy_channel(float* y, const float* x, int n, int c, int hw, int ch, float alpha, hipStream_t stream) {
  SRPDE_CHECK_ARG(y && x && n > 0 && ch >= 0 && ch < c && hw > 0, "srpde_axpy_channel: bad args");
  hipLaunchKernelGGL(axpy_channel_kernel, dim3(grid_for((long long)n * hw)), dim3(256), 0, stream, y, x, n, c, hw, ch,
                     alpha);
  SRPDE_LAUNCH_CHECK("srpde_axpy_channel");
  return 0;
}

int srpde_maxpool2x2_fwd(const float* x, int ldx, float* out, int ldo, int n, int h, int w, int c,
                         hipStream_t stream) {
  SRPDE_CHECK_ARG(x && out && c % 4 == 0 && h % 2 == 0 && w % 2 == 0, "srpde_maxpool2x2_fwd: bad args");
  launch_px_or_grid_stride(
      (long long)n * (h / 2) * (w / 2), c,
      [&](dim3 g, dim3 b, unsigned npix) {
        hipLaunchKernelGGL(maxpool2_fwd_px_kernel, g, b, 0, stream, x, ldx, out, ldo, npix, h, w);
      },
      [&](dim3 g) { hipLaunchKernelGGL(maxpool2_fwd_kernel, g, dim3(256), 0, stream, x, ldx, out, ldo, n, h, w, c); });
  SRPDE_LAUNCH_CHECK("srpde_maxpool2x2_fwd");
  return 0;
}

int srpde_maxpool2x2_bwd(const float* x, int ldx, const float* dout, int lddo, float* dx, int lddx, int n, int h,
                         int w, int c, int accumulate, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && dout && dx && c % 4 == 0 && h % 2 == 0 && w % 2 == 0, "srpde_maxpool2x2_bwd: bad args");
  launch_px_or_grid_stride(
      (long long)n * (h / 2) * (w / 2), c,
      [&](dim3 g, dim3 b, unsigned npix) {
        hipLaunchKernelGGL(maxpool2_bwd_px_kernel, g, b, 0, stream, x, ldx, dout, lddo, dx, lddx, npix, h, w, accumulate);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL(maxpool2_bwd_kernel, g, dim3(256), 0, stream, x, ldx, dout, lddo, dx, lddx, n, h, w, c,
                           accumulate);
      });
  SRPDE_LAUNCH_CHECK("srpde_maxpool2x2_bwd");
  return 0;
}

int srpde_pde_dataset_assemble(const float* u_coarse, const float* u_fine, const float* theta_fine,
                               const float* f_fine, const float* stats, int theta_constant, int n, int hc, int wc,
                               int hf, int wf, float* inputs, float* targets, hipStream_t stream) {
  SRPDE_CHECK_ARG(u_coarse && u_fine && theta_fine && f_fine && stats && inputs && targets,
                  "srpde_pde_dataset_assemble: null");
  SRPDE_CHECK_ARG(n >= 0 && hc >= 1 && wc >= 1 && hf >= hc && wf >= wc, "srpde_pde_dataset_assemble: bad shape");
  if (n == 0) return 0;
  hipLaunchKernelGGL(pde_dataset_kernel, dim3(grid_for((long long)n * hf * wf)), dim3(256), 0, stream, u_coarse,
                     u_fine, theta_fine, f_fine, stats, theta_constant, n, hc, wc, hf, wf, inputs, targets);
  SRPDE_LAUNCH_CHECK("srpde_pde_dataset_assemble");
  return 0;
}

int srpde_upsample_bilinear_fwd(const float* x, int ldx, float* out, int ldo, int n, int h, int w, int ho, int wo,
                                int c, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && out && c > 0, "srpde_upsample_bilinear_fwd: bad args");
  if (c % 4 != 0 || ldx % 4 != 0 || ldo % 4 != 0) {
    hipLaunchKernelGGL(upsample_fwd_scalar_kernel, dim3(grid_for((long long)n * ho * wo * c)), dim3(256), 0, stream,
                       x, ldx, out, ldo, n, h, w, ho, wo, c);
    SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_fwd");
    return 0;
  }
  launch_px_or_grid_stride(
      (long long)n * ho * wo, c,
      [&](dim3 g, dim3 b, unsigned npix) {
        hipLaunchKernelGGL(upsample_fwd_px_kernel, g, b, 0, stream, x, ldx, out, ldo, npix, h, w, ho, wo);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL(upsample_fwd_kernel, g, dim3(256), 0, stream, x, ldx, out, ldo, n, h, w, ho, wo, c);
      });
  SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_fwd");
  return 0;
}

int srpde_upsample_bilinear_gate_fwd(const float* x, int ldx, float* out, int ldo, int n, int h, int w, int ho,
                                      int wo, int c, const float* wg, const float* bg, float* sa, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && out && wg && bg && sa && ldx % 4 == 0 && ldo % 4 == 0 && c % 4 == 0 && c / 4 >= 1 &&
                      c / 4 <= 64 && ((c / 4) & (c / 4 - 1)) == 0,
                  "srpde_upsample_bilinear_gate_fwd: bad args (c / 4 a power of two <= 64)");
  dim3 g, b;
  SRPDE_CHECK_ARG(px_geometry((long long)n * ho * wo, c, &g, &b), "srpde_upsample_bilinear_gate_fwd: bad geometry");
  g.x = (g.x + UPX - 1) / UPX;
  hipLaunchKernelGGL(upsample_gate_fwd_px_kernel, g, b, 0, stream, x, ldx, out, ldo, (unsigned)(n * ho * wo), h, w,
                     ho, wo, wg, bg, sa);
  SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_gate_fwd");
  return 0;
}

size_t srpde_upsample_gate_sa_workspace_size(int n, int h, int w) { return (size_t)n * h * w * sizeof(float); }

int srpde_upsample_gate_sa(const float* x, int ldx, int n, int h, int w, int ho, int wo, int c, const float* wg,
                           const float* bg, float* sa, void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && wg && bg && sa && workspace && ldx % 4 == 0 && c % 4 == 0 && c / 4 >= 1 && c / 4 <= 64 &&
                      ((c / 4) & (c / 4 - 1)) == 0 && n > 0 && h > 0 && w > 0 && ho > 0 && wo > 0,
                  "srpde_upsample_gate_sa: bad args (c / 4 a power of two <= 64)");
  SRPDE_CHECK_ARG(ws_bytes >= srpde_upsample_gate_sa_workspace_size(n, h, w), "srpde_upsample_gate_sa: workspace");
  float* t = static_cast<float*>(workspace);
  dim3 g, b;
  SRPDE_CHECK_ARG(px_geometry((long long)n * h * w, c, &g, &b), "srpde_upsample_gate_sa: bad geometry");
  hipLaunchKernelGGL(gate_dot_px_kernel, g, b, 0, stream, x, ldx, (unsigned)(n * h * w), wg, t);
  SRPDE_LAUNCH_CHECK("srpde_upsample_gate_sa(dot)");
  const unsigned np = (unsigned)(n * ho * wo);
  hipLaunchKernelGGL(up_sigmoid_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, t, sa, np, h, w, ho, wo, bg);
  SRPDE_LAUNCH_CHECK("srpde_upsample_gate_sa(up)");
  return 0;
}

// LDS of the per-sample attention kernels: [256] float4 partials, then C and C / 8 floats
static size_t att_lds_bytes(int c) { return (4 * 256 + c + c / 8) * sizeof(float); }

static void launch_att_channel(const float* x, int ldx, int n, int hw, int c, const float* w1, const float* b1,
                               const float* w2, const float* b2, float* m, float* hbuf, float* ca, hipStream_t stream) {
  hipLaunchKernelGGL(att_channel_fwd_kernel, dim3(n), dim3(256), att_lds_bytes(c), stream, x, ldx, hw, c, c / 8, w1, b1,
                     w2, b2, m, hbuf, ca);
}
static void launch_att_spatial(const float* g, int ldg, long long P, int gc, const float* wg, const float* bg, float* sa,
                               hipStream_t stream) {
  hipLaunchKernelGGL(att_spatial_fwd_kernel, dim3(grid_for(P * 8)), dim3(256), 0, stream, g, ldg, P, gc, wg, bg, sa);
}
static void launch_att_apply(const float* x, int ldx, const float* ca, const float* sa, float* out, int ldo, long long P,
                             int hw, int c, hipStream_t stream) {
  hipLaunchKernelGGL(att_apply_kernel, dim3(grid_for(P * (c / 4))), dim3(256), 0, stream, x, ldx, ca, sa, out, ldo, P,
                     hw, c);
}

int srpde_att_apply_fwd(const float* x, int ldx, int n, int hw, int c, const float* ca, const float* sa, float* out,
                        int ldo, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && ca && sa && out && c % 4 == 0, "srpde_att_apply_fwd: bad args");
  launch_att_apply(x, ldx, ca, sa, out, ldo, (long long)n * hw, hw, c, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_apply_fwd");
  return 0;
}

int srpde_upsample_bilinear_bwd_gated(const float* dout, int lddo, const float* dsa, const float* wg, float* dx,
                                      int lddx, int n, int h, int w, int ho, int wo, int c, int accumulate,
                                      hipStream_t stream) {
  SRPDE_CHECK_ARG(dout && dsa && wg && dx && c % 4 == 0 && lddo % 4 == 0 && lddx % 4 == 0 && ho >= h && wo >= w,
                  "srpde_upsample_bilinear_bwd_gated: bad args");
  SRPDE_CHECK_ARG(upsample_gather_ok(h, ho) && upsample_gather_ok(w, wo),
                  "srpde_upsample_bilinear_bwd_gated: upsampling ratio above 4 (%dx%d -> %dx%d)", h, w, ho, wo);
  if (upsample_rows_ok(h, w, ho, wo, c, lddo, lddx)) {
    launch_upsample_bwd_rows<true>(dout, lddo, dx, lddx, n, h, w, ho, wo, c, accumulate, dsa, wg, stream);
    SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_bwd_gated");
    return 0;
  }
  dim3 g, b;
  SRPDE_CHECK_ARG(px_geometry((long long)n * h * w, c, &g, &b),
                  "srpde_upsample_bilinear_bwd_gated: needs c / 4 a power of two <= 256 (c=%d)", c);
  hipLaunchKernelGGL(upsample_bwd_px_kernel, g, b, 0, stream, dout, lddo, dx, lddx, (unsigned)(n * h * w), h, w, ho,
                     wo, accumulate, dsa, wg);
  SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_bwd_gated");
  return 0;
}

int srpde_upsample_bwd_bn_supported(int h, int w, int ho, int wo, int c, int lddo, int lddx) {
  return upsample_gather_ok(h, ho) && upsample_gather_ok(w, wo) && upsample_rows_ok(h, w, ho, wo, c, lddo, lddx) ? 1
                                                                                                               : 0;
}

int srpde_upsample_bilinear_bwd_gated_bn(const float* dout, int lddo, const float* dsa, const float* wg, float* dx,
                                         int lddx, int n, int h, int w, int ho, int wo, int c, const float* y, int ldy,
                                         const float* mean, const float* invstd, const float* gamma,
                                         const float* beta, int flags, void* part, float* da_max,
                                         hipStream_t stream) {
  SRPDE_CHECK_ARG(dout && dsa && wg && dx && y && mean && invstd && gamma && beta && part && da_max && ldy % 4 == 0 &&
                      aligned16(y) && aligned16(dx) && aligned16(dout),
                  "srpde_upsample_bilinear_bwd_gated_bn: null argument / alignment");
  SRPDE_CHECK_ARG(ho >= h && wo >= w && srpde_upsample_bwd_bn_supported(h, w, ho, wo, c, lddo, lddx),
                  "srpde_upsample_bilinear_bwd_gated_bn: shape outside the row-blocked kernel "
                  "(srpde_upsample_bwd_bn_supported)");
  const UpBnArgs bn{y, ldy, mean, invstd, gamma, beta, flags & SRPDE_BN_RELU, static_cast<float2*>(part), da_max};
  launch_upsample_bwd_rows<true>(dout, lddo, dx, lddx, n, h, w, ho, wo, c, 0, dsa, wg, stream, &bn);
  SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_bwd_gated_bn");
  return 0;
}

int srpde_upsample_bilinear_bwd(const float* dout, int lddo, float* dx, int lddx, int n, int h, int w, int ho,
                                int wo, int c, int accumulate, hipStream_t stream) {
  SRPDE_CHECK_ARG(dout && dx && c % 4 == 0 && ho >= h && wo >= w, "srpde_upsample_bilinear_bwd: bad args");
  SRPDE_CHECK_ARG(upsample_gather_ok(h, ho) && upsample_gather_ok(w, wo),
                  "srpde_upsample_bilinear_bwd: upsampling ratio above 4 (%dx%d -> %dx%d)", h, w, ho, wo);
  if (upsample_rows_ok(h, w, ho, wo, c, lddo, lddx)) {
    launch_upsample_bwd_rows<false>(dout, lddo, dx, lddx, n, h, w, ho, wo, c, accumulate, nullptr, nullptr, stream);
    SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_bwd");
    return 0;
  }
  launch_px_or_grid_stride(
      (long long)n * h * w, c,
      [&](dim3 g, dim3 b, unsigned npix) {
        hipLaunchKernelGGL(upsample_bwd_px_kernel, g, b, 0, stream, dout, lddo, dx, lddx, npix, h, w, ho, wo, accumulate);
      },
      [&](dim3 g) {
        hipLaunchKernelGGL(upsample_bwd_kernel, g, dim3(256), 0, stream, dout, lddo, dx, lddx, n, h, w, ho, wo, c,
                           accumulate);
      });
  SRPDE_LAUNCH_CHECK("srpde_upsample_bilinear_bwd");
  return 0;
}

int srpde_att_channel_fwd(const float* x, int ldx, int n, int hw, int c, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* m, float* hbuf, float* ca, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && w1 && b1 && w2 && b2 && m && hbuf && ca, "srpde_att_channel_fwd: null");
  SRPDE_CHECK_ARG(c % 32 == 0 && c <= 1024, "srpde_att_channel_fwd: channel count");
  launch_att_channel(x, ldx, n, hw, c, w1, b1, w2, b2, m, hbuf, ca, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_channel_fwd");
  return 0;
}

int srpde_att_gate_fwd(const float* x, int ldx, const float* g, int ldg, int n, int hw, int c, int gc,
                       const float* ca, const float* wg, const float* bg, float* sa, float* out, int ldo,
                       hipStream_t stream) {
  SRPDE_CHECK_ARG(x && g && ca && wg && bg && sa && out, "srpde_att_gate_fwd: null");
  SRPDE_CHECK_ARG(c % 32 == 0 && gc % 4 == 0 && c <= 1024, "srpde_att_gate_fwd: channel counts");
  const long long P = (long long)n * hw;
  launch_att_spatial(g, ldg, P, gc, wg, bg, sa, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_gate_fwd(spatial)");
  launch_att_apply(x, ldx, ca, sa, out, ldo, P, hw, c, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_gate_fwd(apply)");
  return 0;
}

int srpde_att_fwd(const float* x, int ldx, const float* g, int ldg, int n, int hw, int c, int gc, const float* w1,
                  const float* b1, const float* w2, const float* b2, const float* wg, const float* bg, float* m,
                  float* hbuf, float* ca, float* sa, float* out, int ldo, hipStream_t stream) {
  SRPDE_CHECK_ARG(x && g && w1 && b1 && w2 && b2 && wg && bg && m && hbuf && ca && sa && out,
                  "srpde_att_fwd: null");
  SRPDE_CHECK_ARG(c % 32 == 0 && gc % 4 == 0 && c <= 1024, "srpde_att_fwd: channel counts");
  launch_att_channel(x, ldx, n, hw, c, w1, b1, w2, b2, m, hbuf, ca, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_fwd(channel)");
  const long long P = (long long)n * hw;
  launch_att_spatial(g, ldg, P, gc, wg, bg, sa, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_fwd(spatial)");
  launch_att_apply(x, ldx, ca, sa, out, ldo, P, hw, c, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_fwd(apply)");
  return 0;
}

size_t srpde_att_bwd_workspace_size(int n, int hw, int c, int gc) {
  if (!att_bwd_counts_ok(c, gc)) return 0;   // the entries reject such counts
  const long long P = (long long)n * hw;
  const int cr = c / 8;
  int rpb;
  const int nb = colsum_blocks(P, gc, &rpb);
  size_t f = (size_t)P                          // dsa_pre
             + (size_t)n * c                    // dm
             + (size_t)n * cr * c * 2           // dw1 rows, dw2 rows
             + (size_t)n * (cr + c)             // db1, db2 rows
             + (size_t)nb * (gc + 1) * 2;       // float2 partials
  return f * sizeof(float) + 256;
}

int srpde_att_bwd(const float* dout, int lddo, const float* x, int ldx, const float* g, int ldg, int n, int hw,
                  int c, int gc, const float* w1, const float* w2, const float* wg, const float* m, const float* hbuf,
                  const float* ca, const float* sa, float* dx, int lddx, int dx_accumulate, float* dg, int lddg,
                  int dg_accumulate, float* dw1, float* db1, float* dw2, float* db2, float* dwg, float* dbg,
                  void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(dout && x && g && workspace, "srpde_att_bwd: null");
  SRPDE_CHECK_ARG(att_bwd_counts_ok(c, gc), "srpde_att_bwd: channel counts (c %% 32, gc %% 4, both <= 1024)");
  if (ws_bytes < srpde_att_bwd_workspace_size(n, hw, c, gc)) {
    set_error("srpde_att_bwd: workspace too small");
    return kErrWorkspace;
  }
  const long long P = (long long)n * hw;
  const int cr = c / 8;
  float* dsa = static_cast<float*>(workspace);
  float* dm = dsa + P;
  float* dw1r = dm + (size_t)n * c;
  float* dw2r = dw1r + (size_t)n * cr * c;
  float* db1r = dw2r + (size_t)n * cr * c;
  float* db2r = db1r + (size_t)n * cr;
  float2* part = reinterpret_cast<float2*>(db2r + (size_t)n * c + 2);
  part = reinterpret_cast<float2*>((reinterpret_cast<uintptr_t>(part) + 15) & ~uintptr_t(15));

  const size_t lds = att_lds_bytes(c);
  if (c == 64 || c == 128 || c == 256) {   // one pass over dout and x per sample
    hipLaunchKernelGGL(att_bwd_sample_kernel, dim3(n), dim3(256), lds, stream, dout, lddo, x, ldx, sa, hw, c, cr, w1,
                       w2, m, hbuf, ca, dm, dw1r, db1r, dw2r, db2r, dsa);
    SRPDE_LAUNCH_CHECK("srpde_att_bwd(sample)");
  } else {
    hipLaunchKernelGGL(att_bwd_pixel_kernel, dim3(grid_for(P * 8)), dim3(256), 0, stream, dout, lddo, x, ldx, ca,
                       sa, P, hw, c, dsa);
    SRPDE_LAUNCH_CHECK("srpde_att_bwd(pixel)");
    hipLaunchKernelGGL(att_bwd_channel_kernel, dim3(n), dim3(256), lds, stream, dout, lddo, x, ldx, sa, hw, c, cr,
                       w1, w2, m, hbuf, ca, dm, dw1r, db1r, dw2r, db2r);
    SRPDE_LAUNCH_CHECK("srpde_att_bwd(channel)");
  }
  if (dx != nullptr) {   // else the caller forms dx later from workspace's dm (srpde_att_pool_bn_bwd)
    hipLaunchKernelGGL(att_bwd_dx_kernel, dim3(grid_for(P * (c / 4))), dim3(256), 0, stream, dout, lddo, ca, sa, dm,
                       dx, lddx, P, hw, c, dx_accumulate);
    SRPDE_LAUNCH_CHECK("srpde_att_bwd(dx)");
  }
  if (dg != nullptr) {   // else the caller folds dg = dsa * wg into its consumer (workspace[0, P) = dsa)
    hipLaunchKernelGGL(att_bwd_gating_kernel, dim3(grid_for(P * (gc / 4))), dim3(256), 0, stream, dsa, wg, dg, lddg,
                       P, gc, dg_accumulate);
    SRPDE_LAUNCH_CHECK("srpde_att_bwd(gating)");
  }
  if (dw1 == nullptr) return 0;   // parameter gradients later: srpde_att_bwd_params
  return srpde_att_bwd_params(g, ldg, n, hw, c, gc, m, hbuf, dw1, db1, dw2, db2, dwg, dbg, workspace, ws_bytes,
                              stream);
}

// sT[q] = sum of w(p, q) dsa[p] over the output pixels p that interpolate from low-res pixel q: the transpose of the
// bilinear x2 upsample (align_corners, models.py:89 / :92) on one channel, each low-res pixel gathering its
// candidate rows and columns in a fixed order (upsample_bwd_rows_kernel's candidate test)
__global__ __launch_bounds__(256) void upsample_t_scalar_kernel(const float* __restrict__ dsa, float* __restrict__ st,
                                                                int n, int h, int w, int ho, int wo) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long long)n * h * w) return;
  const int ix = (int)(q % w), iy = (int)((q / w) % h), nn = (int)(q / ((long long)w * h));
  int ylo, yhi, xlo, xhi;
  cand_range(iy, h, ho, &ylo, &yhi);
  cand_range(ix, w, wo, &xlo, &xhi);
  const float* base = dsa + (size_t)nn * ho * wo;
  float s = 0.f;
  for (int oy = ylo; oy <= yhi; ++oy) {
    bool hy;
    const float wy = cand_weight(oy, iy, h, ho, &hy);
    if (!hy) continue;
    float r = 0.f;
    for (int ox = xlo; ox <= xhi; ++ox) {
      bool hx;
      const float wx = cand_weight(ox, ix, w, wo, &hx);
      if (hx) r += wx * base[(size_t)oy * wo + ox];
    }
    s += wy * r;
  }
  st[q] = s;
}

// the channel MLP's parameter gradients of srpde_att_bwd_params (fixed-order sums over samples)
static void att_params_outer(int n, int c, const float* m, const float* hbuf, const float* db1r, const float* db2r,
                             float* dw1, float* db1, float* dw2, float* db2, hipStream_t stream) {
  const int cr = c / 8;
  // dW1[r][c] = sum_n dh[n][r] m[n][c];  dW2[c][r] = sum_n dpre[n][c] h[n][r]
  hipLaunchKernelGGL(outer_sum_kernel, dim3(cr, ceil_div(c, 64)), dim3(1024), 0, stream, db1r, cr, m, c, n, dw1);
  hipLaunchKernelGGL(outer_sum_kernel, dim3(c, ceil_div(cr, 64)), dim3(1024), 0, stream, db2r, c, hbuf, cr, n, dw2);
  hipLaunchKernelGGL(outer_sum_kernel, dim3(1, ceil_div(cr, 64)), dim3(1024), 0, stream, (const float*)nullptr, 1,
                     db1r, cr, n, db1);
  hipLaunchKernelGGL(outer_sum_kernel, dim3(1, ceil_div(c, 64)), dim3(1024), 0, stream, (const float*)nullptr, 1,
                     db2r, c, n, db2);
}

int srpde_att_bwd_params_lowres(const float* d, int ldd, int n, int h, int w, int ho, int wo, int c, int gc,
                                const float* m, const float* hbuf, float* dw1, float* db1, float* dw2, float* db2,
                                float* dwg, float* dbg, void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(d && m && hbuf && dw1 && db1 && dw2 && db2 && dwg && dbg && workspace && ldd % 4 == 0 && ho >= h &&
                      wo >= w,
                  "srpde_att_bwd_params_lowres: bad args");
  SRPDE_CHECK_ARG(att_bwd_counts_ok(c, gc),
                  "srpde_att_bwd_params_lowres: channel counts (c %% 32, gc %% 4, both <= 1024)");
  const int hw = ho * wo;
  if (ws_bytes < srpde_att_bwd_workspace_size(n, hw, c, gc)) {
    set_error("srpde_att_bwd_params_lowres: workspace too small");
    return kErrWorkspace;
  }
  const long long P = (long long)n * hw, Plo = (long long)n * h * w;
  const int cr = c / 8;
  float* dsa = static_cast<float*>(workspace);
  float* dm = dsa + P;
  float* dw1r = dm + (size_t)n * c;
  float* dw2r = dw1r + (size_t)n * cr * c;
  float* db1r = dw2r + (size_t)n * cr * c;
  float* db2r = db1r + (size_t)n * cr;
  float2* part = reinterpret_cast<float2*>(db2r + (size_t)n * c + 2);
  part = reinterpret_cast<float2*>((reinterpret_cast<uintptr_t>(part) + 15) & ~uintptr_t(15));
  SRPDE_CHECK_ARG(Plo <= 2LL * n * cr * c, "srpde_att_bwd_params_lowres: low-res field larger than its scratch");
  float* st = dw1r;   // the per-sample MLP rows' region, unused by the parameter pass
  att_params_outer(n, c, m, hbuf, db1r, db2r, dw1, db1, dw2, db2, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd_params_lowres(rowsum)");
  // dwg[k] = sum_p dsa[p] up(d)[p][k] = sum_q d[q][k] sT[q]; dbg = sum_p dsa[p] = sum_q sT[q] (the weights of an
  // output pixel sum to 1): the weighted column sums run over the low-res d, 1/4 of up(d)'s rows
  hipLaunchKernelGGL(upsample_t_scalar_kernel, dim3((unsigned)((Plo + 255) / 256)), dim3(256), 0, stream, dsa, st, n, h,
                     w, ho, wo);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd_params_lowres(transpose)");
  int rpb;
  const int nb = colsum_blocks(Plo, gc, &rpb);
  hipLaunchKernelGGL(weighted_colsum_kernel, dim3(nb), dim3(256), 2 * 256 * sizeof(float4), stream, d, ldd, st, Plo,
                     gc, rpb, part);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd_params_lowres(colsum)");
  hipLaunchKernelGGL(partsum_kernel, dim3(gc), dim3(256), 0, stream, part, nb, gc + 1, dwg);
  hipLaunchKernelGGL(partsum_kernel, dim3(1), dim3(256), 0, stream, part + gc, nb, gc + 1, dbg);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd_params_lowres(partsum)");
  return 0;
}

int srpde_att_bwd_params(const float* g, int ldg, int n, int hw, int c, int gc, const float* m, const float* hbuf,
                         float* dw1, float* db1, float* dw2, float* db2, float* dwg, float* dbg, void* workspace,
                         size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(g && m && hbuf && dw1 && db1 && dw2 && db2 && dwg && dbg && workspace,
                  "srpde_att_bwd_params: null");
  SRPDE_CHECK_ARG(att_bwd_counts_ok(c, gc), "srpde_att_bwd_params: channel counts (c %% 32, gc %% 4, both <= 1024)");
  if (ws_bytes < srpde_att_bwd_workspace_size(n, hw, c, gc)) {
    set_error("srpde_att_bwd_params: workspace too small");
    return kErrWorkspace;
  }
  const long long P = (long long)n * hw;
  const int cr = c / 8;
  float* dsa = static_cast<float*>(workspace);
  float* dm = dsa + P;
  float* dw1r = dm + (size_t)n * c;
  float* dw2r = dw1r + (size_t)n * cr * c;
  float* db1r = dw2r + (size_t)n * cr * c;
  float* db2r = db1r + (size_t)n * cr;
  float2* part = reinterpret_cast<float2*>(db2r + (size_t)n * c + 2);
  part = reinterpret_cast<float2*>((reinterpret_cast<uintptr_t>(part) + 15) & ~uintptr_t(15));
  // parameter grads: fixed-order sums over samples / pixel blocks
  (void)dw1r; (void)dw2r; (void)cr;
  att_params_outer(n, c, m, hbuf, db1r, db2r, dw1, db1, dw2, db2, stream);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd(rowsum)");
  int rpb;
  const int nb = colsum_blocks(P, gc, &rpb);
  hipLaunchKernelGGL(weighted_colsum_kernel, dim3(nb), dim3(256), 2 * 256 * sizeof(float4), stream, g, ldg, dsa, P,
                     gc, rpb, part);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd(colsum)");
  hipLaunchKernelGGL(partsum_kernel, dim3(gc), dim3(256), 0, stream, part, nb, gc + 1, dwg);
  hipLaunchKernelGGL(partsum_kernel, dim3(1), dim3(256), 0, stream, part + gc, nb, gc + 1, dbg);
  SRPDE_LAUNCH_CHECK("srpde_att_bwd(partsum)");
  return 0;
}

int srpde_head_fwd(const float* z, int ldz, int c, const float* wf, const float* bf, const float* xin, int xin_c,
                   int n, int hw, float* out, hipStream_t stream) {
  SRPDE_CHECK_ARG(z && wf && bf && xin && out && c % 4 == 0, "srpde_head_fwd: bad args");
  const long long P = (long long)n * hw;
  hipLaunchKernelGGL(head_fwd_kernel, dim3(grid_for(P)), dim3(256), 0, stream, z, ldz, c, wf, bf, xin, xin_c, hw, P,
                     out);
  SRPDE_LAUNCH_CHECK("srpde_head_fwd");
  return 0;
}

size_t srpde_head_bwd_workspace_size(int n, int hw, int c) {
  if (!colsum_ok(c)) return 0;   // srpde_head_bwd rejects such counts
  int rpb;
  const int nb = colsum_blocks((long long)n * hw, c, &rpb);
  return (size_t)nb * (c + 1) * sizeof(float2);
}

int srpde_head_bwd(const float* dout, const float* z, int ldz, int c, const float* wf, int n, int hw, float* dz,
                   int lddz, float* dwf, float* dbf, void* workspace, size_t ws_bytes, hipStream_t stream) {
  SRPDE_CHECK_ARG(dout && z && wf && dz && dwf && dbf && workspace, "srpde_head_bwd: bad args");
  SRPDE_CHECK_ARG(colsum_ok(c), "srpde_head_bwd: channel count (c %% 4, 4 <= c <= 1024)");
  if (ws_bytes < srpde_head_bwd_workspace_size(n, hw, c)) {
    set_error("srpde_head_bwd: workspace too small");
    return kErrWorkspace;
  }
  const long long P = (long long)n * hw;
  hipLaunchKernelGGL(head_bwd_dz_kernel, dim3(grid_for(P * (c / 4))), dim3(256), 0, stream, dout, wf, c, dz, lddz, P);
  SRPDE_LAUNCH_CHECK("srpde_head_bwd(dz)");
  int rpb;
  const int nb = colsum_blocks(P, c, &rpb);
  float2* part = static_cast<float2*>(workspace);
  hipLaunchKernelGGL(weighted_colsum_kernel, dim3(nb), dim3(256), 2 * 256 * sizeof(float4), stream, z, ldz, dout, P,
                     c, rpb, part);
  hipLaunchKernelGGL(partsum_kernel, dim3(c), dim3(256), 0, stream, part, nb, c + 1, dwf);
  hipLaunchKernelGGL(partsum_kernel, dim3(1), dim3(256), 0, stream, part + c, nb, c + 1, dbf);
  SRPDE_LAUNCH_CHECK("srpde_head_bwd(reduce)");
  return 0;
}

size_t srpde_mse_workspace_size(void) { return 1024 * sizeof(double); }

int srpde_mse_fwd(const float* y, const float* t, long long n, float* loss, void* workspace, size_t ws_bytes,
                  hipStream_t stream) {
  SRPDE_CHECK_ARG(y && t && loss && workspace && ws_bytes >= 1024 * sizeof(double), "srpde_mse_fwd: bad args");
  const int nb = (int)std::min<long long>(1024, std::max<long long>(1, (n + 255) / 256));
  hipLaunchKernelGGL(mse_partial_kernel, dim3(nb), dim3(256), 0, stream, y, t, n, static_cast<double*>(workspace));
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, stream, static_cast<const double*>(workspace), nb, n,
                     loss);
  SRPDE_LAUNCH_CHECK("srpde_mse_fwd");
  return 0;
}

int srpde_mse_bwd(const float* y, const float* t, long long n, const float* gout, float* dy, hipStream_t stream) {
  SRPDE_CHECK_ARG(y && t && dy, "srpde_mse_bwd: bad args");
  hipLaunchKernelGGL(mse_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, stream, y, t, n, gout, dy);
  SRPDE_LAUNCH_CHECK("srpde_mse_bwd");
  return 0;
}

}  // extern "C"
