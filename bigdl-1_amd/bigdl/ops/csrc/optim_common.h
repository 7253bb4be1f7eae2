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

// shadow[4i .. 4i+3] = bf16(w), one 8-B store
__device__ __forceinline__ void store_shadow4(bf16_t* shadow, long long i, const float (&w)[4]) {
  const uint32_t lo = (uint32_t)f2bf(w[0]) | ((uint32_t)f2bf(w[1]) << 16);
  const uint32_t hi = (uint32_t)f2bf(w[2]) | ((uint32_t)f2bf(w[3]) << 16);
  reinterpret_cast<uint2*>(shadow)[i] = make_uint2(lo, hi);
}
