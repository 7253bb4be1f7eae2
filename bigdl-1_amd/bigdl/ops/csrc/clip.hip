// Σg² of a gradient range for L2-norm gradient clipping (DL/parameters/ParameterOperations.scala:89):
// the one global quantity the clipped update kernels (GradClip, optim_common.h) read from the device.
//
//   k_grad_sumsq       grid-stride pass, one partial per workgroup  -> partials[block]
//   k_grad_sumsq_fold  one wave                                     -> out[0] = sum of the partials
//
// The store-pass-plus-sum-pass form of a cross-workgroup reduction (cdna_hip_programming.md
// Guideline 12), as the LARS layer sums in lars.hip: no float atomics, every addition in a fixed
// order, so out[0] is bitwise identical from run to run.  HBM-bound: 16 B per lane per access for an
// fp32 gradient, 8 B for the bf16 wire shard (widened on load), grid capped at 2048 blocks of 256.
#include "optim_common.h"

#define SUMSQ_GRID_CAP 2048

// Addition depth D of out[0] for n elements on a grid of G = min(2048, ceil((n/4) / 256)) blocks
// (every term is a non-negative square, so the relative error is at most D * 2^-24; a square is
// formed inside its fused multiply-add and adds no rounding of its own):
//   per lane, four independent accumulators each take I = ceil((n/4) / (256 G)) terms, and one of
//   them one more for the n & 3 tail (block 0);
//   2 levels to join the four, 6 levels of the wave64 butterfly, 2 levels across the 4 waves (LDS);
//   the fold adds ceil(G / 64) partials per lane, then 6 butterfly levels:
//   D = I + 1 + 2 + 6 + 2 + ceil(G / 64) + 6.
// n <= 2^21 + 3 gives I = 1 and D <= 50; the 25.6 M-element ResNet-50 arena gives I = 13, D = 62.
template <typename GT>
__global__ void __launch_bounds__(256) k_grad_sumsq(const GT* __restrict__ g, long long n4, int tail,
                                                    float* __restrict__ partials) {
  const int t = threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * blockDim.x + t; i < n4; i += stride) {
    float gv[4];
    g_load4(g, i, gv);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = fmaf(gv[k], gv[k], a[k]);
  }
  if (blockIdx.x == 0 && t < tail) {
    // the n % 4 trailing elements, scalar, like k_sgd's tail
    const float gg = g_at(g, n4 * 4 + t);
    a[1] = fmaf(gg, gg, a[1]);
  }
  const float sw = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  __shared__ float sm[4];
  if ((t & 63) == 0) sm[t >> 6] = sw;
  __syncthreads();
  if (t == 0) partials[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ void __launch_bounds__(64) k_grad_sumsq_fold(const float* __restrict__ partials, int np,
                                                        float* __restrict__ out) {
  const int t = threadIdx.x;
  float a = 0.f;
  for (int i = t; i < np; i += 64) a += partials[i];
  a = wave_sum(a);
  if (t == 0) out[0] = a;
}

template <typename GT>
static int grad_sumsq_impl(const GT* g, long long n, float* partials, int grid, float* out, hipStream_t s) {
  hipLaunchKernelGGL((k_grad_sumsq<GT>), dim3(grid), dim3(256), 0, s, g, n / 4, (int)(n & 3), partials);
  hipLaunchKernelGGL(k_grad_sumsq_fold, dim3(1), dim3(64), 0, s, (const float*)partials, grid, out);
  BIGDL_CHECK_LAUNCH();
}

// g: n elements, fp32 (16-B aligned) or, with g16, bf16 (8-B aligned); partials: npartials floats of
// scratch owned by the caller, at least one per workgroup (2048 always suffice); out: fp32 [1].
// n == 0 gives out[0] = 0.
BIGDL_EXPORT int bigdl_grad_sumsq(const void* g, int g16, long long n, float* partials, int npartials, float* out,
                                  hipStream_t s) {
  if (n < 0 || !partials || !out) return (int)hipErrorInvalidValue;
  if (n > 0 && (!g || ((uintptr_t)g & (g16 ? 7 : 15)))) return (int)hipErrorInvalidValue;
  const long long n4 = n / 4;
  const int grid = bigdl_grid(n4 > 0 ? n4 : 1, 256, SUMSQ_GRID_CAP);
  if (npartials < grid) return (int)hipErrorInvalidValue;
  if (g16) return grad_sumsq_impl((const bf16_t*)g, n, partials, grid, out, s);
  return grad_sumsq_impl((const float*)g, n, partials, grid, out, s);
}
