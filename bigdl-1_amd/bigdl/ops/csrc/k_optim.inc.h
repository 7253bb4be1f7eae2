// The body of k_optim, included twice by optim_rules.hip: as k_optim (K_OPTIM_CLIP 0), whose text — and
// so whose code and bits — is what it was before gradient clipping existed, and as k_optim_clip
// (K_OPTIM_CLIP 1) with a GradClip operand (optim_common.h): the gradient is clamped and L2-scaled
// right after the load with the 1/N scale (cscale) inside the clip; the launcher sets the rule's own
// scale to 1.  A shared __device__ body was tried first: inlined, it changed which product of
// g*scale + wd*w the compiler fused, and with it the bits of the unclipped Adam and Adagrad updates.
template <typename R, typename G>
__global__ void K_OPTIM_NAME(R r, float* __restrict__ w, const G* __restrict__ g, float* __restrict__ s0,
                        float* __restrict__ s1, bf16_t* __restrict__ shadow, long long n4, int tail K_OPTIM_CLIP_PARAMS) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  r.prepare();
#if K_OPTIM_CLIP
  const ClipFn clip(c, cscale);
#endif
  if (blockIdx.x == 0 && threadIdx.x < tail) {
    const long long e = n4 * 4 + threadIdx.x;
    float nw = w[e], a = s0[e], b = 0.f;
    if (R::NS > 1) b = s1[e];
#if K_OPTIM_CLIP
    r.step(nw, clip(g_at(g, e)), a, b);
#else
    r.step(nw, g_at(g, e), a, b);
#endif
    w[e] = nw;
    s0[e] = a;
    if (R::NS > 1) s1[e] = b;
    if (shadow) shadow[e] = f2bf(nw);
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 W = reinterpret_cast<float4*>(w)[i];
    const float4 A = reinterpret_cast<float4*>(s0)[i];
    float wv[4] = {W.x, W.y, W.z, W.w}, gv[4], av[4] = {A.x, A.y, A.z, A.w}, bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (R::NS > 1) {
      const float4 B = reinterpret_cast<float4*>(s1)[i];
      bv[0] = B.x; bv[1] = B.y; bv[2] = B.z; bv[3] = B.w;
    }
    g_load4(g, i, gv);
#if K_OPTIM_CLIP
#pragma unroll
    for (int k = 0; k < 4; ++k) gv[k] = clip(gv[k]);
#endif
#pragma unroll
    for (int k = 0; k < 4; ++k) r.step(wv[k], gv[k], av[k], bv[k]);
    reinterpret_cast<float4*>(w)[i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
    reinterpret_cast<float4*>(s0)[i] = make_float4(av[0], av[1], av[2], av[3]);
    if (R::NS > 1) reinterpret_cast<float4*>(s1)[i] = make_float4(bv[0], bv[1], bv[2], bv[3]);
    if (shadow) store_shadow4(shadow, i, wv);
  }
}
