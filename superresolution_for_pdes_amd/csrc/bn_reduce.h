// The BatchNorm (+ ReLU) backward reduction: sum dz and sum dz * xhat per channel, dz = d * [bn_out > 0], and
// max|d|, as float2 partials per block.  bn_bwd_reduce_kernel, gating_bn_reduce_kernel, att_pool_bn_bwd_kernel
// (bn.hip) and upsample_bwd_rows_kernel<., true> (pointwise.hip) all form them here, so a gradient reduced by
// the pass that writes it gives the bits of the separate reduction pass.
#pragma once
#include "vec4.h"

namespace srpde {

// xhat of a conv output v, and d behind the ReLU mask of bn_out = xhat * g + b.  relu bit 0: a ReLU follows
// the BN; ALWAYS: the kernel has no flag, its BN is always followed by one
template <bool ALWAYS = false>
__device__ __forceinline__ float bn_relu_mask(float v, float mu, float is, float g, float b, float d, int relu,
                                              float* xhat) {
  const float xh = (v - mu) * is;
  *xhat = xh;
  return ((!ALWAYS && !(relu & 1)) || xh * g + b > 0.f) ? d : 0.f;
}

// one channel's step: t1 += dz, t2 += dz * xhat
template <bool ALWAYS>
__device__ __forceinline__ void bn_bwd_add1(float v, float mu, float is, float g, float b, float d, int relu, float& t1,
                                            float& t2) {
  float xh;
  const float dz = bn_relu_mask<ALWAYS>(v, mu, is, g, b, d, relu, &xh);
  t1 += dz;
  t2 += dz * xh;
}

// one thread's share of the reduction for its channel quad
struct BnBwdAcc {
  float4 mu, is, g, b;
  float4 s1 = zero4(), s2 = zero4();
  float dmax = 0.f;

  __device__ __forceinline__ void load(const float* mean, const float* invstd, const float* gamma, const float* beta,
                                       int c) {
    mu = ld4(mean + c);
    is = ld4(invstd + c);
    g = ld4(gamma + c);
    b = ld4(beta + c);
  }
  // the BN's input quad y and its output gradient quad d
  template <bool ALWAYS = false>
  __device__ __forceinline__ void add(const float4& y, const float4& d, int relu = 1) {
    bn_bwd_add1<ALWAYS>(y.x, mu.x, is.x, g.x, b.x, d.x, relu, s1.x, s2.x);
    bn_bwd_add1<ALWAYS>(y.y, mu.y, is.y, g.y, b.y, d.y, relu, s1.y, s2.y);
    bn_bwd_add1<ALWAYS>(y.z, mu.z, is.z, g.z, b.z, d.z, relu, s1.z, s2.z);
    bn_bwd_add1<ALWAYS>(y.w, mu.w, is.w, g.w, b.w, d.w, relu, s1.w, s2.w);
  }
  __device__ __forceinline__ void amax(const float4& d) { dmax = fmaxf(dmax, absmax4(d)); }
};

// the block's partials from sums[2][256] (sum dz, then sum dz * xhat, one quad per thread slot [nrows][C4]):
// channel quad q's rows summed in row order -> o[0..3]
__device__ __forceinline__ void bn_bwd_store_part(const float4* sums, int C4, int nrows, int q, float2* o) {
  float4 t1 = zero4(), t2 = t1;
  for (int r = 0; r < nrows; ++r) {
    t1 = add4(t1, sums[r * C4 + q]);
    t2 = add4(t2, sums[256 + r * C4 + q]);
  }
  store_part4(o, t1, t2);
}
__device__ __forceinline__ float max4slots(const float* wmx) { return fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3])); }

// A 256-thread block's combine, red4 [2][256] float4 of LDS: thread tid (its slot: row * C4 + quad) hands in its
// sums, the threads `lead` (row 0; quad q) write the block's partials to o, and with want_max (block-uniform)
// the four waves' maxima go through the start of red4 to *da_max.
__device__ __forceinline__ void bn_bwd_block_combine(float4* red4, int tid, bool lead, int q, int C4, int nrows,
                                                     const BnBwdAcc& acc, float2* o, bool want_max, float* da_max) {
  red4[tid] = acc.s1;
  red4[256 + tid] = acc.s2;
  __syncthreads();
  if (lead) bn_bwd_store_part(red4, C4, nrows, q, o);
  if (want_max) {
    const float dmax = wave_max(acc.dmax);
    __syncthreads();
    float* wmx = reinterpret_cast<float*>(red4);
    if ((tid & 63) == 0) wmx[tid >> 6] = dmax;
    __syncthreads();
    if (tid == 0) *da_max = max4slots(wmx);
  }
}

}  // namespace srpde
