// Channel concat for training (K19): one-launch concat forward, fused split + ReLU-mask backward,
// and the K-way gradient sum.  All three are HBM-bound streaming kernels on a rows x channels view
// (dense NHWC, or a 2-D [N, C]): 16 B per lane per access (8 bf16 or 4 fp32), 64-bit chunk index,
// grid-stride, 256 threads, grid capped at 2048 blocks (cdna_hip_programming.md Guideline 11).
// Plain vector loads and stores only.
#include "common.h"

#define BIGDL_CAT_MAX 8

// One part of a concat: channels [c0, c0 + c) of the wide tensor <-> a contiguous [M][c] tensor.
struct CatPart {
  void* p;   // the part's tensor (16-B aligned, checked on the host)
  int c0;    // first channel in the wide tensor
  int c;     // channels (a multiple of the vector width, checked on the host)
  int flag;  // split backward: 1 = apply the ReLU mask y > 0
  int pad_;
};

// Passed by value.  The launch covers channels [lo, lo + span) of every row; parts are sorted by c0
// and tile that range exactly (checked by the launcher).
struct CatTable {
  CatPart part[BIGDL_CAT_MAX];
  int n;
  int lo;
  int span;
  int ctot;
};

template <typename T> struct CatVec;
template <> struct CatVec<bf16_t> { static constexpr int W = 8; };
template <> struct CatVec<float> { static constexpr int W = 4; };

// The part holding channel cc: the last one whose offset is <= cc.  Unrolled selects over the
// by-value table (kernel arguments), so no dynamically indexed private array.
__device__ __forceinline__ void cat_find(const CatTable& t, int cc, char*& p, int& c0, int& c, int& flag) {
  p = (char*)t.part[0].p; c0 = t.part[0].c0; c = t.part[0].c; flag = t.part[0].flag;
#pragma unroll
  for (int k = 1; k < BIGDL_CAT_MAX; ++k) {
    if (k < t.n && cc >= t.part[k].c0) {
      p = (char*)t.part[k].p; c0 = t.part[k].c0; c = t.part[k].c; flag = t.part[k].flag;
    }
  }
}

// y[row][cc .. cc+W) = part[row][cc - c0 .. )
template <typename T>
__global__ void __launch_bounds__(256) k_concat_fwd(CatTable t, T* __restrict__ y, long long M) {
  constexpr int W = CatVec<T>::W;
  const long long cpr = t.span / W, total = M * cpr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long row = i / cpr;
    const int cc = t.lo + (int)(i - row * cpr) * W;
    char* p; int c0, c, flag;
    cat_find(t, cc, p, c0, c, flag);
    const uint4 v = *reinterpret_cast<const uint4*>((const T*)p + row * c + (cc - c0));
    *reinterpret_cast<uint4*>(y + row * t.ctot + cc) = v;
  }
}

__device__ __forceinline__ uint4 cat_mask(uint4 g, uint4 y, const bf16_t*) {
  // bf16 > 0 <=> sign clear and magnitude non-zero and not NaN; as a float compare on the widened value
  const uint32_t gw[4] = {g.x, g.y, g.z, g.w}, yw[4] = {y.x, y.y, y.z, y.w};
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = __uint_as_float(yw[k] << 16) > 0.f ? (gw[k] & 0xFFFFu) : 0u;
    const uint32_t hi = __uint_as_float(yw[k] & 0xFFFF0000u) > 0.f ? (gw[k] & 0xFFFF0000u) : 0u;
    o[k] = lo | hi;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ uint4 cat_mask(uint4 g, uint4 y, const float*) {
  g.x = __uint_as_float(y.x) > 0.f ? g.x : 0u;
  g.y = __uint_as_float(y.y) > 0.f ? g.y : 0u;
  g.z = __uint_as_float(y.z) > 0.f ? g.z : 0u;
  g.w = __uint_as_float(y.w) > 0.f ? g.w : 0u;
  return g;
}

// part[row][..] = flag ? (y > 0 ? gy : 0) : gy — a select on the stored bits, never a multiply, so
// the result has the bits of relu_backward(split(gy), y_slice, 0)
template <typename T>
__global__ void __launch_bounds__(256) k_concat_split_bwd(CatTable t, const T* __restrict__ gy,
                                                          const T* __restrict__ y, long long M) {
  constexpr int W = CatVec<T>::W;
  const long long cpr = t.span / W, total = M * cpr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long row = i / cpr;
    const int cc = t.lo + (int)(i - row * cpr) * W;
    char* p; int c0, c, flag;
    cat_find(t, cc, p, c0, c, flag);
    const long long off = row * t.ctot + cc;
    uint4 g = *reinterpret_cast<const uint4*>(gy + off);
    if (flag) g = cat_mask(g, *reinterpret_cast<const uint4*>(y + off), (const T*)nullptr);
    *reinterpret_cast<uint4*>((T*)p + row * c + (cc - c0)) = g;
  }
}

static int cat_check(const CatTable& t, long long M, int W) {
  if (M <= 0 || t.n < 1 || t.n > BIGDL_CAT_MAX || t.span <= 0 || t.lo < 0 || t.ctot % W || t.lo % W ||
      t.lo + t.span > t.ctot)
    return 0;
  int c = t.lo;
  for (int k = 0; k < t.n; ++k) {
    const CatPart& q = t.part[k];
    if (q.c0 != c || q.c <= 0 || q.c % W || !q.p || ((uintptr_t)q.p & 15)) return 0;
    c += q.c;
  }
  return c == t.lo + t.span;
}

// parts -> channels [lo, lo+span) of y[M][ctot].  dtype 0 = bf16, 1 = fp32.
BIGDL_EXPORT int bigdl_concat_fwd(const CatTable* tab, void* y, long long M, int dtype, hipStream_t s) {
  const CatTable t = *tab;
  const int W = dtype ? 4 : 8;
  if (!cat_check(t, M, W) || !y || ((uintptr_t)y & 15)) return (int)hipErrorInvalidValue;
  const int grid = bigdl_grid(M * (t.span / W), 256);
  if (dtype)
    hipLaunchKernelGGL(k_concat_fwd<float>, dim3(grid), dim3(256), 0, s, t, (float*)y, M);
  else
    hipLaunchKernelGGL(k_concat_fwd<bf16_t>, dim3(grid), dim3(256), 0, s, t, (bf16_t*)y, M);
  BIGDL_CHECK_LAUNCH();
}

// channels [lo, lo+span) of gy[M][ctot] -> parts; y (the forward output, same layout) is read where a
// part's flag is set and may be null when none is.
BIGDL_EXPORT int bigdl_concat_split_bwd(const CatTable* tab, const void* gy, const void* y, long long M, int dtype,
                                        hipStream_t s) {
  const CatTable t = *tab;
  const int W = dtype ? 4 : 8;
  if (!cat_check(t, M, W) || !gy || ((uintptr_t)gy & 15) || ((uintptr_t)y & 15)) return (int)hipErrorInvalidValue;
  for (int k = 0; k < t.n; ++k)
    if (t.part[k].flag && !y) return (int)hipErrorInvalidValue;
  const int grid = bigdl_grid(M * (t.span / W), 256);
  if (dtype)
    hipLaunchKernelGGL(k_concat_split_bwd<float>, dim3(grid), dim3(256), 0, s, t, (const float*)gy, (const float*)y,
                       M);
  else
    hipLaunchKernelGGL(k_concat_split_bwd<bf16_t>, dim3(grid), dim3(256), 0, s, t, (const bf16_t*)gy,
                       (const bf16_t*)y, M);
  BIGDL_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------
// K-way sum
// ------------------------------------------------------------------------------------------------
struct SumPtrs {
  const void* p[BIGDL_CAT_MAX];
  int n;
  int pad_;
};

// out = (((a0 + a1) + a2) + ...) — added left to right in fp32 and ROUNDED TO THE STORAGE DTYPE AFTER
// EVERY ADD.  That is exactly what the chain of pairwise tensor adds it replaces computes (each bf16
// add is an fp32 add rounded to bf16), so the result is bit-identical to it; a single rounding at the
// end would be more accurate but would change the training numerics (in bf16, 1 + 2^-8 + 2^-8 is 1
// per add — each a tie that rounds to even — and 1.0078125 with one rounding).
__global__ void __launch_bounds__(256) k_sum_n_bf16(SumPtrs a, bf16_t* __restrict__ out, long long n) {
  const long long n8 = n >> 3, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    float acc[8], v[8];
    load8((const bf16_t*)a.p[0] + 8 * i, acc);
#pragma unroll
    for (int k = 1; k < BIGDL_CAT_MAX; ++k) {
      if (k < a.n) {
        load8((const bf16_t*)a.p[k] + 8 * i, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = bf2f(f2bf(acc[j] + v[j]));
      }
    }
    store8(out + 8 * i, acc);
  }
  for (long long i = (n8 << 3) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float acc = bf2f(((const bf16_t*)a.p[0])[i]);
#pragma unroll
    for (int k = 1; k < BIGDL_CAT_MAX; ++k)
      if (k < a.n) acc = bf2f(f2bf(acc + bf2f(((const bf16_t*)a.p[k])[i])));
    out[i] = f2bf(acc);
  }
}

__global__ void __launch_bounds__(256) k_sum_n_f32(SumPtrs a, float* __restrict__ out, long long n) {
  const long long n4 = n >> 2, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 acc = reinterpret_cast<const float4*>(a.p[0])[i];
#pragma unroll
    for (int k = 1; k < BIGDL_CAT_MAX; ++k) {
      if (k < a.n) {
        const float4 v = reinterpret_cast<const float4*>(a.p[k])[i];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    reinterpret_cast<float4*>(out)[i] = acc;
  }
  for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float acc = ((const float*)a.p[0])[i];
#pragma unroll
    for (int k = 1; k < BIGDL_CAT_MAX; ++k)
      if (k < a.n) acc += ((const float*)a.p[k])[i];
    out[i] = acc;
  }
}

// 2 <= K <= 8 dense tensors of n elements each (16-B aligned, checked on the host too)
BIGDL_EXPORT int bigdl_sum_n(const SumPtrs* ptrs, void* out, long long n, int dtype, hipStream_t s) {
  const SumPtrs a = *ptrs;
  if (n <= 0) return 0;
  if (a.n < 2 || a.n > BIGDL_CAT_MAX || !out || ((uintptr_t)out & 15)) return (int)hipErrorInvalidValue;
  for (int k = 0; k < a.n; ++k)
    if (!a.p[k] || ((uintptr_t)a.p[k] & 15)) return (int)hipErrorInvalidValue;
  const int W = dtype ? 4 : 8;
  const int grid = bigdl_grid((n + W - 1) / W, 256);
  if (dtype)
    hipLaunchKernelGGL(k_sum_n_f32, dim3(grid), dim3(256), 0, s, a, (float*)out, n);
  else
    hipLaunchKernelGGL(k_sum_n_bf16, dim3(grid), dim3(256), 0, s, a, (bf16_t*)out, n);
  BIGDL_CHECK_LAUNCH();
}
