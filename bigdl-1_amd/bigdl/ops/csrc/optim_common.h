// What every update kernel (k_sgd, k_optim, the LARS pair) shares: the gradient loaders and the
// four-float bf16 shadow store.  A gradient is fp32 (16-B aligned) or the bf16 reduce-scatter
// output of the bf16 wire format (8-B aligned), widened on load, so no kernel needs a separate
// unpack pass over the shard.  Index i counts groups of four elements.
#pragma once
#include "common.h"

__device__ __forceinline__ float g_at(const float* g, long long e) { return g[e]; }
__device__ __forceinline__ float g_at(const bf16_t* g, long long e) { return bf2f(g[e]); }
__device__ __forceinline__ void g_load4(const float* g, long long i, float (&o)[4]) {
  const float4 G = reinterpret_cast<const float4*>(g)[i];
  o[0] = G.x; o[1] = G.y; o[2] = G.z; o[3] = G.w;
}
__device__ __forceinline__ void g_load4(const bf16_t* g, long long i, float (&o)[4]) {
  const uint2 G = reinterpret_cast<const uint2*>(g)[i];
  o[0] = __uint_as_float(G.x << 16); o[1] = __uint_as_float(G.x & 0xffff0000u);
  o[2] = __uint_as_float(G.y << 16); o[3] = __uint_as_float(G.y & 0xffff0000u);
}

// Gradient clipping as an operand of the update kernels (the _clip entry points): what
// run_processors([ConstantClipping, L2NormClipping]) does to g·scale, term for term.
struct GradClip {
  const float* sumsq;  // fp32 [1] on the device: Σg² of the RAW gradient over all ranks; null = no L2 clip
  float threshold;     // l2NormThreshold
  float lo, hi;        // constant clamp; -inf / +inf = none
};

// The per-thread form: g' = clamp(g·scale, lo, hi)·s with s = min(1, threshold / (‖g‖·scale + 1e-6)),
// the norm taken before the clamp.  The rule that follows runs with scale 1.  Contraction is off
// here so that g·scale is rounded once, as the torch form rounds it, whatever consumes the result.
struct ClipFn {
  float scale, lo, hi, s;
  __device__ __forceinline__ ClipFn(const GradClip& c, float scale_) : scale(scale_), lo(c.lo), hi(c.hi), s(1.f) {
#pragma clang fp contract(off)
    if (c.sumsq) {
      const float norm = sqrtf(c.sumsq[0]) * scale_;
      const float q = c.threshold / (norm + 1e-6f);
      s = q > 1.f ? 1.f : q;  // a NaN norm stays NaN, as torch.clamp(max=1) keeps it
    }
  }
  __device__ __forceinline__ float operator()(float g) const {
#pragma clang fp contract(off)
    const float x = g * scale;
    return (x < lo ? lo : (x > hi ? hi : x)) * s;  // a NaN passes through, as torch.clamp passes it
  }
};

// shadow[4i .. 4i+3] = bf16(w), one 8-B store
__device__ __forceinline__ void store_shadow4(bf16_t* shadow, long long i, const float (&w)[4]) {
  const uint32_t lo = (uint32_t)f2bf(w[0]) | ((uint32_t)f2bf(w[1]) << 16);
  const uint32_t hi = (uint32_t)f2bf(w[2]) | ((uint32_t)f2bf(w[3]) << 16);
  reinterpret_cast<uint2*>(shadow)[i] = make_uint2(lo, hi);
}
