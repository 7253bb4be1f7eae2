// Layer-wise adaptive rate scaling (DL/optim/LarsSGD.scala:47) over a flat update space (the
// parameter arena, or one rank's shard of it) described by a chunk table built once on the host:
//
//   chunk c = elements [start[c], start[c] + len[c]) of layer layer[c]; no chunk crosses a layer
//   boundary or leaves the range this rank owns.  Starts and lengths are arbitrary, so every kernel
//   peels a scalar head up to the next multiple of 4 elements, moves 16 B per lane over the aligned
//   body (the array bases are 16-B aligned, host-checked; 8 B for a bf16 gradient / shadow) and
//   finishes with a scalar tail, like k_sgd's tail.
//
//   bigdl_lars_sumsq  one workgroup per chunk -> partials[c] = (sum w^2, sum g^2)
//   bigdl_lars_fold   one wave per layer      -> sums[l]     = sum of its chunks' partials
//   bigdl_lars_sgd    one workgroup per chunk -> the momentum-SGD update at the layer's LARS rate
//
// sumsq + fold are the store-pass-plus-sum-pass form of a cross-workgroup reduction
// (cdna_hip_programming.md Guideline 12): no float atomics, every addition in a fixed order, so the
// sums are bitwise identical from run to run.
#include "optim_common.h"

// head / aligned body / tail of a chunk: head = elements before the next multiple of 4
struct Split {
  long long s;     // first element
  int head;        // scalar elements at s
  long long i4;    // first float4 index of the body
  int n4;          // float4s in the body
  int tail;        // scalar elements after the body
};

__device__ __forceinline__ Split split_chunk(long long s, int n) {
  Split p;
  p.s = s;
  int h = (int)((4 - (s & 3)) & 3);
  p.head = h < n ? h : n;
  p.i4 = (s + p.head) >> 2;
  p.n4 = (n - p.head) >> 2;
  p.tail = n - p.head - 4 * p.n4;
  return p;
}

// Addition depth of one layer sum (every term is a non-negative square, so the relative error is
// at most depth * 2^-24): per lane, four independent accumulators each take chunk/(4*256) terms
// (8 at the 8192-element chunk the plan uses) plus at most one head and one tail term; then 2
// levels to join the four, 6 levels of the wave64 butterfly, 2 levels across the 4 waves through
// LDS; the fold adds ceil(chunks/64) terms per lane and 6 butterfly levels.  A square is formed
// inside its fused multiply-add, so it adds no rounding of its own: the depth is
// 8 + 2 + 2 + 6 + 2 + 1 + 6 = 27 for a layer of up to 64 chunks.
template <typename GT>
__global__ void __launch_bounds__(256) k_lars_sumsq(const float* __restrict__ w, const GT* __restrict__ g,
                                                    const long long* __restrict__ cstart,
                                                    const int* __restrict__ clen, float* __restrict__ partials) {
  const int c = blockIdx.x, t = threadIdx.x;
  const Split p = split_chunk(cstart[c], clen[c]);
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ag[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = t; i < p.n4; i += 256) {
    const float4 W = reinterpret_cast<const float4*>(w)[p.i4 + i];
    float gv[4];
    g_load4(g, p.i4 + i, gv);
    aw[0] = fmaf(W.x, W.x, aw[0]); aw[1] = fmaf(W.y, W.y, aw[1]);
    aw[2] = fmaf(W.z, W.z, aw[2]); aw[3] = fmaf(W.w, W.w, aw[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) ag[k] = fmaf(gv[k], gv[k], ag[k]);
  }
  if (t < p.head) {
    const float wv = w[p.s + t], gg = g_at(g, p.s + t);
    aw[1] = fmaf(wv, wv, aw[1]);
    ag[1] = fmaf(gg, gg, ag[1]);
  }
  if (t < p.tail) {
    const long long e = p.s + p.head + 4ll * p.n4 + t;
    const float wv = w[e], gg = g_at(g, e);
    aw[2] = fmaf(wv, wv, aw[2]);
    ag[2] = fmaf(gg, gg, ag[2]);
  }
  float sw = wave_sum((aw[0] + aw[1]) + (aw[2] + aw[3]));
  float sg = wave_sum((ag[0] + ag[1]) + (ag[2] + ag[3]));
  __shared__ float sm[2][4];
  if ((t & 63) == 0) {
    sm[0][t >> 6] = sw;
    sm[1][t >> 6] = sg;
  }
  __syncthreads();
  if (t == 0) {
    partials[2 * c] = (sm[0][0] + sm[0][1]) + (sm[0][2] + sm[0][3]);
    partials[2 * c + 1] = (sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]);
  }
}

// layer l owns the chunk ids lchunks[lptr[l] .. lptr[l+1]) (a layer may have several pieces on this
// rank, or none: its sums are then exactly 0)
__global__ void __launch_bounds__(64) k_lars_fold(const float* __restrict__ partials, const int* __restrict__ lptr,
                                                  const int* __restrict__ lchunks, float* __restrict__ sums) {
  const int l = blockIdx.x, t = threadIdx.x;
  float a = 0.f, b = 0.f;
  for (int i = lptr[l] + t; i < lptr[l + 1]; i += 64) {
    const int c = lchunks[i];
    a += partials[2 * c];
    b += partials[2 * c + 1];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (t == 0) {
    sums[2 * l] = a;
    sums[2 * l + 1] = b;
  }
}

// hyper row of a layer: (lr * trust, weightDecay, momentum, lr).  The rate follows
// LarsSGD.optimize: ratio = wn / (gn + wd * wn + 1e-12) scaled by trust when both norms are
// positive, else the plain lr (ratio 1, no trust factor).
template <typename GT, bool SHADOW>
__global__ void __launch_bounds__(256) k_lars_sgd(float* __restrict__ w, const GT* __restrict__ g,
                                                  float* __restrict__ v, bf16_t* __restrict__ shadow,
                                                  const long long* __restrict__ cstart, const int* __restrict__ clen,
                                                  const int* __restrict__ clayer, const float* __restrict__ sums,
                                                  const float* __restrict__ hyper, int c0, float scale) {
  const int c = c0 + blockIdx.x, t = threadIdx.x;
  const int l = clayer[c];
  const float lrt = hyper[4 * l], wd = hyper[4 * l + 1], mom = hyper[4 * l + 2], lr = hyper[4 * l + 3];
  const float wn = sqrtf(sums[2 * l]);
  const float gn = scale * sqrtf(sums[2 * l + 1]);
  const float rate = (wn > 0.f && gn > 0.f) ? lrt * (wn / (gn + wd * wn + 1e-12f)) : lr;
  const Split p = split_chunk(cstart[c], clen[c]);
  for (int i = t; i < p.n4; i += 256) {
    const long long j = p.i4 + i;
    const float4 W = reinterpret_cast<float4*>(w)[j];
    const float4 B = reinterpret_cast<float4*>(v)[j];
    float wv[4] = {W.x, W.y, W.z, W.w}, bv[4] = {B.x, B.y, B.z, B.w}, gv[4];
    g_load4(g, j, gv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bv[k] = mom * bv[k] + rate * (gv[k] * scale + wd * wv[k]);
      wv[k] -= bv[k];
    }
    reinterpret_cast<float4*>(w)[j] = make_float4(wv[0], wv[1], wv[2], wv[3]);
    reinterpret_cast<float4*>(v)[j] = make_float4(bv[0], bv[1], bv[2], bv[3]);
    if (SHADOW) store_shadow4(shadow, j, wv);
  }
  // scalar head (lanes 0..head-1) and tail (lanes 64..64+tail-1, another wave)
  long long e = -1;
  if (t < p.head) e = p.s + t;
  else if (t >= 64 && t - 64 < p.tail) e = p.s + p.head + 4ll * p.n4 + (t - 64);
  if (e >= 0) {
    const float wv = w[e];
    const float b = mom * v[e] + rate * (g_at(g, e) * scale + wd * wv);
    const float nw = wv - b;
    v[e] = b;
    w[e] = nw;
    if (SHADOW) shadow[e] = f2bf(nw);
  }
}

template <typename GT>
static int lars_sumsq_impl(const float* w, const GT* g, const long long* cstart, const int* clen, int nchunks,
                           float* partials, hipStream_t s) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL((k_lars_sumsq<GT>), dim3(nchunks), dim3(256), 0, s, w, g, cstart, clen, partials);
  BIGDL_CHECK_LAUNCH();
}

template <typename GT>
static int lars_sgd_impl(float* w, const GT* g, float* v, bf16_t* shadow, const long long* cstart, const int* clen,
                         const int* clayer, const float* sums, const float* hyper, int c0, int c1, float scale,
                         hipStream_t s) {
  if (c1 <= c0) return 0;
  if (shadow)
    hipLaunchKernelGGL((k_lars_sgd<GT, true>), dim3(c1 - c0), dim3(256), 0, s, w, g, v, shadow, cstart, clen, clayer,
                       sums, hyper, c0, scale);
  else
    hipLaunchKernelGGL((k_lars_sgd<GT, false>), dim3(c1 - c0), dim3(256), 0, s, w, g, v, shadow, cstart, clen, clayer,
                       sums, hyper, c0, scale);
  BIGDL_CHECK_LAUNCH();
}

// w 16-B aligned; g 16-B (fp32) or 8-B (bf16) aligned; the table was range-checked against the
// space when it was built and the wrapper checks the tensors against the table.
BIGDL_EXPORT int bigdl_lars_sumsq(const float* w, const void* g, int g16, const long long* cstart, const int* clen,
                                  int nchunks, float* partials, hipStream_t s) {
  if (g16) return lars_sumsq_impl<bf16_t>(w, (const bf16_t*)g, cstart, clen, nchunks, partials, s);
  return lars_sumsq_impl<float>(w, (const float*)g, cstart, clen, nchunks, partials, s);
}

// second pass of the layer sums: [2 * nlayers] floats, one wave per layer
BIGDL_EXPORT int bigdl_lars_fold(const float* partials, const int* lptr, const int* lchunks, int nlayers, float* sums,
                                 hipStream_t s) {
  if (nlayers <= 0) return 0;
  hipLaunchKernelGGL(k_lars_fold, dim3(nlayers), dim3(64), 0, s, partials, lptr, lchunks, sums);
  BIGDL_CHECK_LAUNCH();
}

// chunks [c0, c1) of the table; v is the momentum buffer over the same space
BIGDL_EXPORT int bigdl_lars_sgd(float* w, const void* g, int g16, float* v, bf16_t* shadow, const long long* cstart,
                                const int* clen, const int* clayer, const float* sums, const float* hyper, int c0,
                                int c1, float scale, hipStream_t s) {
  if (g16)
    return lars_sgd_impl<bf16_t>(w, (const bf16_t*)g, v, shadow, cstart, clen, clayer, sums, hyper, c0, c1, scale, s);
  return lars_sgd_impl<float>(w, (const float*)g, v, shadow, cstart, clen, clayer, sums, hyper, c0, c1, scale, s);
}
