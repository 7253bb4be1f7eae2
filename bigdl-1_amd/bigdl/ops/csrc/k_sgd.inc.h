// The body of k_sgd, included twice by elementwise.hip: as k_sgd (K_SGD_CLIP 0), whose text — and so
// whose code and bits — is what it was before gradient clipping existed, and as k_sgd_clip
// (K_SGD_CLIP 1) with a GradClip operand (optim_common.h): the gradient is clamped and L2-scaled
// right after the load with the 1/N scale inside the clip, and the update runs with scale = one
// (1, passed at run time so that the multiply-add below keeps its shape).
// A shared __device__ body was tried first: inlined, it changed which product of g*scale + wd*w the
// compiler fused, and with it the bits of the unclipped update.
template <typename GT, bool MOM, bool NEST, bool FIRST, bool SHADOW, bool PERELEM>
__global__ void K_SGD_NAME(float* __restrict__ w, const GT* __restrict__ g, float* __restrict__ buf,
                      bf16_t* __restrict__ shadow, const float* __restrict__ lrs, const float* __restrict__ wds,
                      long long n4, float lr, float mom, float damp, float wd, float scale, int tail,
                      const float* __restrict__ first_dev K_SGD_CLIP_PARAMS) {
  long long stride = (long long)gridDim.x * blockDim.x;
#if K_SGD_CLIP
  const ClipFn clip(c, scale);
  scale = one;
#endif
  // first-iteration rule (v = g) from the template or, in HIP-graph mode, from a device flag the
  // captured step clears after the update (so a replayed graph can start a fresh trajectory)
  const bool first = FIRST || (first_dev != nullptr && *first_dev != 0.f);
  if (blockIdx.x == 0 && threadIdx.x < tail) {
    // the n % 4 trailing elements (scalar; the arena slice need not be a multiple of 4)
    const long long e = n4 * 4 + threadIdx.x;
    const float wv = w[e];
#if K_SGD_CLIP
    const float gg = clip(g_at(g, e)) * scale + wd * (PERELEM && wds ? wds[e] : 1.f) * wv;
#else
    const float gg = g_at(g, e) * scale + wd * (PERELEM && wds ? wds[e] : 1.f) * wv;
#endif
    float d = gg;
    if (MOM) {
      const float b = first ? gg : mom * buf[e] + (1.f - damp) * gg;
      buf[e] = b;
      d = NEST ? gg + mom * b : b;
    }
    const float nw = wv - lr * (PERELEM && lrs ? lrs[e] : 1.f) * d;
    w[e] = nw;
    if (SHADOW) shadow[e] = f2bf(nw);
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 W = reinterpret_cast<float4*>(w)[i];
    float wv[4] = {W.x, W.y, W.z, W.w};
    float gv[4];
    g_load4(g, i, gv);
#if K_SGD_CLIP
#pragma unroll
    for (int k = 0; k < 4; ++k) gv[k] = clip(gv[k]);
#endif
    float wdv[4] = {1.f, 1.f, 1.f, 1.f};
    float lrv[4] = {1.f, 1.f, 1.f, 1.f};
    if (PERELEM) {
      if (wds) {
        float4 t = reinterpret_cast<const float4*>(wds)[i];
        wdv[0] = t.x; wdv[1] = t.y; wdv[2] = t.z; wdv[3] = t.w;
      }
      if (lrs) {
        float4 t = reinterpret_cast<const float4*>(lrs)[i];
        lrv[0] = t.x; lrv[1] = t.y; lrv[2] = t.z; lrv[3] = t.w;
      }
    }
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (MOM && !first) {
      float4 B = reinterpret_cast<float4*>(buf)[i];
      bv[0] = B.x; bv[1] = B.y; bv[2] = B.z; bv[3] = B.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gg = gv[k] * scale + wd * wdv[k] * wv[k];
      float d = gg;
      if (MOM) {
        bv[k] = first ? gg : mom * bv[k] + (1.f - damp) * gg;
        d = NEST ? gg + mom * bv[k] : bv[k];
      }
      wv[k] -= lr * lrv[k] * d;
    }
    reinterpret_cast<float4*>(w)[i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
    if (MOM) reinterpret_cast<float4*>(buf)[i] = make_float4(bv[0], bv[1], bv[2], bv[3]);
    if (SHADOW) store_shadow4(shadow, i, wv);
  }
}
