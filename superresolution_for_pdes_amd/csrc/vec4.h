// float4 helpers of the elementwise kernels (bn.hip, pointwise.hip): one channel quad per thread.
// Each keeps the operation order and association of the component-wise text it replaced; the
// results, and with contraction decided after inlining the instructions, are the same.
#pragma once
#include "resample.h"

namespace srpde {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// a + b
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// acc + w * g
__device__ __forceinline__ float4 fma4(const float4& acc, float w, const float4& g) {
  return make_float4(acc.x + w * g.x, acc.y + w * g.y, acc.z + w * g.z, acc.w + w * g.w);
}
// s * w + g (the attention gating gradient s[p] * wg[c] joining a gradient g)
__device__ __forceinline__ float4 scale_add4(float s, const float4& w, const float4& g) {
  return make_float4(s * w.x + g.x, s * w.y + g.y, s * w.z + g.z, s * w.w + g.w);
}
// (d * s) * a + g: the attention gate's input gradient, (dout * sa) * ca + dm
__device__ __forceinline__ float4 gate_dx4(const float4& d, float s, const float4& a, const float4& g) {
  return make_float4((d.x * s) * a.x + g.x, (d.y * s) * a.y + g.y, (d.z * s) * a.z + g.z, (d.w * s) * a.w + g.w);
}
// s * w
__device__ __forceinline__ float4 scale4(float s, const float4& w) {
  return make_float4(s * w.x, s * w.y, s * w.z, s * w.w);
}
__device__ __forceinline__ float4 relu4(const float4& v) {
  return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
// x . w
__device__ __forceinline__ float dot4(const float4& x, const float4& w) {
  return x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w;
}
__device__ __forceinline__ float max4(const float4& v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float absmax4(const float4& v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// nn.MaxPool2d(2) of one window: first maximum in (0,0),(0,1),(1,0),(1,1) order wins (strict >), as aten
__device__ __forceinline__ float max2x2_first(float a, float b, float d, float f) {
  float v = a;
  if (b > v) v = b;
  if (d > v) v = d;
  if (f > v) v = f;
  return v;
}
__device__ __forceinline__ float4 max2x2_first(const float4& a, const float4& b, const float4& d, const float4& f) {
  return make_float4(max2x2_first(a.x, b.x, d.x, f.x), max2x2_first(a.y, b.y, d.y, f.y),
                     max2x2_first(a.z, b.z, d.z, f.z), max2x2_first(a.w, b.w, d.w, f.w));
}

// the window position max2x2_first takes its value from
__device__ __forceinline__ int argmax2x2_first(float v0, float v1, float v2, float v3) {
  int am = 0;
  float mv = v0;
  if (v1 > mv) { mv = v1; am = 1; }
  if (v2 > mv) { mv = v2; am = 2; }
  if (v3 > mv) { mv = v3; am = 3; }
  return am;
}
// max-pool backward of one window: o[argmax of v] += g per channel, by a dynamic index into o
__device__ __forceinline__ void route_argmax(const float4 (&v)[4], const float4& g, float4 (&o)[4]) {
  int am = argmax2x2_first(v[0].x, v[1].x, v[2].x, v[3].x);
  o[am].x += g.x;
  am = argmax2x2_first(v[0].y, v[1].y, v[2].y, v[3].y);
  o[am].y += g.y;
  am = argmax2x2_first(v[0].z, v[1].z, v[2].z, v[3].z);
  o[am].z += g.z;
  am = argmax2x2_first(v[0].w, v[1].w, v[2].w, v[3].w);
  o[am].w += g.w;
}
// the same by selects, for a kernel that keeps o live afterwards (a dynamic index put o in scratch there)
__device__ __forceinline__ void route_select(int am, float g, float& o0, float& o1, float& o2, float& o3) {
  o0 = am == 0 ? o0 + g : o0;
  o1 = am == 1 ? o1 + g : o1;
  o2 = am == 2 ? o2 + g : o2;
  o3 = am == 3 ? o3 + g : o3;
}
__device__ __forceinline__ void route_argmax_select(const float4 (&v)[4], const float4& g, float4 (&o)[4]) {
  route_select(argmax2x2_first(v[0].x, v[1].x, v[2].x, v[3].x), g.x, o[0].x, o[1].x, o[2].x, o[3].x);
  route_select(argmax2x2_first(v[0].y, v[1].y, v[2].y, v[3].y), g.y, o[0].y, o[1].y, o[2].y, o[3].y);
  route_select(argmax2x2_first(v[0].z, v[1].z, v[2].z, v[3].z), g.z, o[0].z, o[1].z, o[2].z, o[3].z);
  route_select(argmax2x2_first(v[0].w, v[1].w, v[2].w, v[3].w), g.w, o[0].w, o[1].w, o[2].w, o[3].w);
}

// bilinear blend of the four source pixels a (i0, i0), b (i0, i1), d (i1, i0), f (i1, i1)
__device__ __forceinline__ float bilerp(const Lerp& ly, const Lerp& lx, float a, float b, float d, float f) {
  return ly.l0 * (lx.l0 * a + lx.l1 * b) + ly.l1 * (lx.l0 * d + lx.l1 * f);
}
__device__ __forceinline__ float4 bilerp4(const Lerp& ly, const Lerp& lx, const float4& a, const float4& b,
                                          const float4& d, const float4& f) {
  return make_float4(bilerp(ly, lx, a.x, b.x, d.x, f.x), bilerp(ly, lx, a.y, b.y, d.y, f.y),
                     bilerp(ly, lx, a.z, b.z, d.z, f.z), bilerp(ly, lx, a.w, b.w, d.w, f.w));
}

// o[0..3] = (t1.c, t2.c) for the quad's four channels: the float2 partial layout of the BN backward reductions
__device__ __forceinline__ void store_part4(float2* o, const float4& t1, const float4& t2) {
  o[0] = make_float2(t1.x, t2.x); o[1] = make_float2(t1.y, t2.y);
  o[2] = make_float2(t1.z, t2.z); o[3] = make_float2(t1.w, t2.w);
}

// sum of rows 0 .. nrows-1 of an LDS block of quads [nrows][C4] at quad q, in row order
__device__ __forceinline__ float4 rowsum4(const float4* red, int C4, int nrows, int q) {
  float4 t = zero4();
  for (int r = 0; r < nrows; ++r) t = add4(t, red[r * C4 + q]);
  return t;
}

}  // namespace srpde
