// K25b: crop → resample (LINEAR / CUBIC) → mirror → per-channel normalise → cast, one launch per batch.
// Packed HWC images (uint8 or fp32, sizes may differ inside a batch) → NHWC bf16 or fp32 — the device form
// of RandomAlterAspect + RandomCropper + ChannelScaledNormalizer + MatToTensor (reference:
// DL/transform/vision/image/augmentation/{RandomAlterAspect,RandomCropper,ChannelScaledNormalizer}.scala).
//
// Rule (per axis, the crop rectangle is an image of its own — OpenCV resize after Crop):
//   s = (o + ½)·n_in/n_out − ½, f = ⌊s⌋, t = s − f, taken from the integers num = (2o+1)·n_in − n_out,
//   den = 2·n_out (f = ⌊num/den⌋, t = rem/den: no float product, so no coordinate rounding);
//   taps f−1…f+2 (CUBIC, A = −0.75) or f, f+1 (LINEAR), clamped to the rectangle; weights are formed in
//   fp64 and rounded once.  The filter is separable: rows are filtered in x, the TAPS results in y, in one
//   fixed fma order shared by both variants below, so they agree to the last bit.
//   CUBIC clamps to [0, 255] (not rounded); then mirror, (v − mean[c])·inv_std[c], cast.
//
// Descriptor row (int64 × 8, one per output image): {byte offset, H, W, y0, x0, ch, cw, flip}.
//
// Two variants, one per launch, picked on the host from the widest / tallest rectangle of the batch:
//  * staged: one workgroup per (image, band of kAugBandRows output rows).  x taps (4 byte offsets + 4 weights
//    per output column) and the band's y taps are formed once into LDS; the source rows the band needs are
//    staged with coalesced dword loads (row pitch W·C is in general no multiple of 4: loads are aligned down
//    and the bytes indexed in LDS); the band's output is staged in LDS and leaves as 16-byte vectors (a band
//    of NHWC rows is one contiguous span), with scalar head/tail where the span's ends are not 16-B aligned.
//  * direct: one thread per output pixel, taps gathered from global memory — any rectangle whose staging
//    would not fit kAugLdsBudget (panoramas, detection inputs).
#include "common.h"

namespace {

// bytes of LDS a workgroup of the staged variant may use: a quarter of a CU's 160 KiB, so that at least four
// workgroups (one wave per SIMD each) stay resident to hide the LDS byte reads of the filter phase
constexpr int kAugLdsBudget = 40 * 1024;
constexpr int kAugBandRows = 8;           // output rows per workgroup (staged variant)
constexpr int kAugThreads = 256;

struct AugParams {
  float mean[4], inv_std[4];
  int C, OH, OW, to_rgb;
};

struct AugRect {
  long long off;
  int H, W, y0, x0, ch, cw, flip;
};

__device__ __forceinline__ AugRect aug_rect(const long long* __restrict__ desc, int b) {
  const long long* d = desc + (long long)b * 8;
  AugRect r;
  r.off = d[0];
  r.H = (int)d[1];
  r.W = (int)d[2];
  r.y0 = (int)d[3];
  r.x0 = (int)d[4];
  r.ch = (int)d[5];
  r.cw = (int)d[6];
  r.flip = (int)d[7];
  return r;
}

// tap indices (clamped to [0, n_in−1]) and weights of output coordinate o
template <int TAPS>
__device__ __forceinline__ void aug_taps(int o, int n_in, int n_out, int* idx, float* w) {
  const long long den = 2LL * n_out;
  const long long num = (2LL * o + 1) * n_in - n_out;
  long long f = num / den, rem = num - f * den;
  if (rem < 0) {
    rem += den;
    --f;
  }
  const double t = (double)rem / (double)den;
  const long long hi = n_in - 1;
  if (TAPS == 4) {
    const double A = -0.75, u = t + 1.0, s = 1.0 - t;
    const double w0 = ((A * u - 5 * A) * u + 8 * A) * u - 4 * A;
    const double w1 = ((A + 2) * t - (A + 3)) * t * t + 1;
    const double w2 = ((A + 2) * s - (A + 3)) * s * s + 1;
    w[0] = (float)w0;
    w[1] = (float)w1;
    w[2] = (float)w2;
    w[3] = (float)(1.0 - w0 - w1 - w2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = f - 1 + k;
      idx[k] = (int)(i < 0 ? 0 : (i > hi ? hi : i));
    }
  } else {
    w[0] = (float)(1.0 - t);
    w[1] = (float)t;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long long i = f + k;
      idx[k] = (int)(i < 0 ? 0 : (i > hi ? hi : i));
    }
  }
}

// rows filtered in x, then the TAPS results in y; `px(r, k)` is the source value of tap row r, tap column k
template <int TAPS, typename PX>
__device__ __forceinline__ float aug_filter(const float* wy, const float* wx, PX px) {
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < TAPS; ++r) {
    float h = 0.f;
#pragma unroll
    for (int k = 0; k < TAPS; ++k) h = __builtin_fmaf(wx[k], px(r, k), h);
    acc = __builtin_fmaf(wy[r], h, acc);
  }
  if (TAPS == 4) acc = fminf(fmaxf(acc, 0.f), 255.f);
  return acc;
}

template <bool OUT_BF16>
__device__ __forceinline__ void aug_put(void* p, long long i, float v) {
  if (OUT_BF16)
    reinterpret_cast<bf16_t*>(p)[i] = f2bf(v);
  else
    reinterpret_cast<float*>(p)[i] = v;
}

// one output pixel, taps read from global memory
template <typename TIN, int TAPS, bool OUT_BF16>
__device__ __forceinline__ void aug_pixel_direct(const uint8_t* __restrict__ src, const AugRect& d,
                                                 const AugParams& P, int b, int oy, int ox,
                                                 void* __restrict__ out) {
  const int C = P.C;
  int iy[4], ix[4];
  float wy[4], wx[4];
  aug_taps<TAPS>(oy, d.ch, P.OH, iy, wy);
  aug_taps<TAPS>(d.flip ? P.OW - 1 - ox : ox, d.cw, P.OW, ix, wx);
  const TIN* rows[TAPS];
#pragma unroll
  for (int r = 0; r < TAPS; ++r)
    rows[r] = reinterpret_cast<const TIN*>(src + d.off) + ((long long)(d.y0 + iy[r]) * d.W + d.x0) * C;
  const long long o = (((long long)b * P.OH + oy) * P.OW + ox) * C;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c >= C) break;
    const int sc = (P.to_rgb && C == 3) ? 2 - c : c;
    const float v = aug_filter<TAPS>(wy, wx, [&](int r, int k) { return (float)rows[r][ix[k] * C + sc]; });
    aug_put<OUT_BF16>(out, o + c, (v - P.mean[c]) * P.inv_std[c]);
  }
}

template <typename TIN, int TAPS, bool OUT_BF16>
__global__ void __launch_bounds__(kAugThreads) k_img_aug_direct(const uint8_t* __restrict__ src,
                                                                const long long* __restrict__ desc, int B,
                                                                AugParams P, void* __restrict__ out) {
  const long long per = (long long)P.OH * P.OW, total = per * B;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total;
       p += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(p / per);
    const int r = (int)(p - (long long)b * per);
    const int oy = r / P.OW;
    aug_pixel_direct<TIN, TAPS, OUT_BF16>(src, aug_rect(desc, b), P, b, oy, r - oy * P.OW, out);
  }
}

__host__ __device__ constexpr int aug_up16(int v) { return (v + 15) & ~15; }

// LDS layout of the staged variant (bytes): x weights | x offsets | y weights | y row bases | output | rows
struct AugLds {
  int xw, xi, yw, yi, so, ss, total;
};

__host__ __device__ inline AugLds aug_lds(int OW, int C, int osz, int rows_cap, int pitch) {
  AugLds l;
  l.xw = 0;
  l.xi = l.xw + OW * 16;
  l.yw = aug_up16(l.xi + OW * 8);
  l.yi = l.yw + kAugBandRows * 16;
  l.so = l.yi + kAugBandRows * 16;
  l.ss = l.so + aug_up16(kAugBandRows * OW * C * osz + 16);
  l.total = l.ss + rows_cap * pitch;
  return l;
}

template <typename TIN, int TAPS, bool OUT_BF16>
__global__ void __launch_bounds__(kAugThreads) k_img_aug_lds(const uint8_t* __restrict__ src, long long src_bytes,
                                                             const long long* __restrict__ desc, int bands,
                                                             AugParams P, int rows_cap, int pitch,
                                                             void* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int ESZ = (int)sizeof(TIN), OSZ = OUT_BF16 ? 2 : 4;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / bands, oy0 = (blockIdx.x - b * bands) * kAugBandRows;
  const int C = P.C, OH = P.OH, OW = P.OW;
  const int nrow = min(kAugBandRows, OH - oy0);
  const AugRect d = aug_rect(desc, b);
  const int seg = d.cw * C * ESZ;

  // source rows of the band (rectangle coordinates): taps are monotone in the output row
  int r_lo, r_hi;
  {
    int idx[4];
    float w[4];
    aug_taps<TAPS>(oy0, d.ch, OH, idx, w);
    r_lo = idx[0];
    aug_taps<TAPS>(oy0 + nrow - 1, d.ch, OH, idx, w);
    r_hi = idx[TAPS - 1];
  }
  const int nr = r_hi - r_lo + 1;
  if (seg + 3 > pitch || nr > rows_cap) {
    // the host sized the launch for a smaller rectangle: gather this band from global memory instead
    for (int i = tid; i < nrow * OW; i += kAugThreads) {
      const int row = i / OW;
      aug_pixel_direct<TIN, TAPS, OUT_BF16>(src, d, P, b, oy0 + row, i - row * OW, out);
    }
    return;
  }

  const AugLds L = aug_lds(OW, C, OSZ, rows_cap, pitch);
  float4* xw = reinterpret_cast<float4*>(smem + L.xw);
  ushort4* xi = reinterpret_cast<ushort4*>(smem + L.xi);
  float4* yw = reinterpret_cast<float4*>(smem + L.yw);
  int4* yi = reinterpret_cast<int4*>(smem + L.yi);
  unsigned char* so = smem + L.so;
  unsigned char* ss = smem + L.ss;

  const long long row_bytes = (long long)d.W * C * ESZ;
  const long long start0 = d.off + ((long long)(d.y0 + r_lo) * d.W + d.x0) * C * ESZ;  // first byte of row r_lo

  for (int ox = tid; ox < OW; ox += kAugThreads) {
    int idx[4] = {0, 0, 0, 0};
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    aug_taps<TAPS>(ox, d.cw, OW, idx, w);
    xw[ox] = make_float4(w[0], w[1], w[2], w[3]);
    xi[ox] = make_ushort4((unsigned short)(idx[0] * C * ESZ), (unsigned short)(idx[1] * C * ESZ),
                          (unsigned short)(idx[2] * C * ESZ), (unsigned short)(idx[3] * C * ESZ));
  }
  if (tid < nrow) {
    int idx[4] = {0, 0, 0, 0};
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    aug_taps<TAPS>(oy0 + tid, d.ch, OH, idx, w);
    int base[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = idx[k] - r_lo;  // staged row; its first byte sits (start & 3) bytes into the LDS row
      base[k] = j * pitch + (int)((start0 + j * row_bytes) & 3);
    }
    yw[tid] = make_float4(w[0], w[1], w[2], w[3]);
    yi[tid] = make_int4(base[0], base[1], base[2], base[3]);
  }
  {
    const int dpr = pitch >> 2;
    uint32_t* sd = reinterpret_cast<uint32_t*>(ss);
    for (int i = tid; i < nr * dpr; i += kAugThreads) {
      const int j = i / dpr, k = i - j * dpr;
      const long long start = start0 + j * row_bytes;
      const long long a = (start & ~3LL) + 4LL * k;
      if (a >= start + seg) continue;
      uint32_t v;
      if (a + 4 <= src_bytes) {
        v = *reinterpret_cast<const uint32_t*>(src + a);
      } else {  // the buffer ends inside this dword
        v = 0;
        for (int q = 0; q < 4; ++q)
          if (a + q < src_bytes) v |= (uint32_t)src[a + q] << (8 * q);
      }
      sd[i] = v;
    }
  }
  __syncthreads();

  const unsigned long long g0 =
      (unsigned long long)out + (unsigned long long)(((long long)b * OH + oy0) * OW) * C * OSZ;
  const int shift = (int)(g0 & 15);  // the LDS image of the span keeps the span's 16-byte phase
  for (int i = tid; i < nrow * OW; i += kAugThreads) {
    const int row = i / OW, ox = i - row * OW;
    const int rx = d.flip ? OW - 1 - ox : ox;
    const float4 wy4 = yw[row], wx4 = xw[rx];
    const int4 yb4 = yi[row];
    const ushort4 xo4 = xi[rx];
    const float wy[4] = {wy4.x, wy4.y, wy4.z, wy4.w}, wx[4] = {wx4.x, wx4.y, wx4.z, wx4.w};
    const int yb[4] = {yb4.x, yb4.y, yb4.z, yb4.w};
    const int xo[4] = {xo4.x, xo4.y, xo4.z, xo4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= C) break;
      const int sc = ((P.to_rgb && C == 3) ? 2 - c : c) * ESZ;
      const float v = aug_filter<TAPS>(
          wy, wx, [&](int r, int k) { return (float)*reinterpret_cast<const TIN*>(ss + yb[r] + xo[k] + sc); });
      aug_put<OUT_BF16>(so + shift, (long long)i * C + c, (v - P.mean[c]) * P.inv_std[c]);
    }
  }
  __syncthreads();

  // the band is one contiguous span of nb bytes: scalar head up to a 16-byte boundary, vectors, scalar tail
  const int nb = nrow * OW * C * OSZ;
  const int head = min((16 - shift) & 15, nb);
  const int nvec = (nb - head) >> 4;
  const int tail0 = head + (nvec << 4);
  unsigned char* g = reinterpret_cast<unsigned char*>(g0);
  const unsigned char* l = so + shift;
  for (int v = tid; v < nvec; v += kAugThreads)
    *reinterpret_cast<uint4*>(g + head + 16 * v) = *reinterpret_cast<const uint4*>(l + head + 16 * v);
  if (OUT_BF16) {
    for (int e = tid; e < (head >> 1); e += kAugThreads)
      reinterpret_cast<bf16_t*>(g)[e] = reinterpret_cast<const bf16_t*>(l)[e];
    for (int e = (tail0 >> 1) + tid; e < (nb >> 1); e += kAugThreads)
      reinterpret_cast<bf16_t*>(g)[e] = reinterpret_cast<const bf16_t*>(l)[e];
  } else {
    for (int e = tid; e < (head >> 2); e += kAugThreads)
      reinterpret_cast<float*>(g)[e] = reinterpret_cast<const float*>(l)[e];
    for (int e = (tail0 >> 2) + tid; e < (nb >> 2); e += kAugThreads)
      reinterpret_cast<float*>(g)[e] = reinterpret_cast<const float*>(l)[e];
  }
}

template <typename TIN, int TAPS, bool OUT_BF16>
int aug_launch(const void* src, long long src_bytes, const long long* desc, int B, const AugParams& P,
               int max_ch, int max_cw, int variant, int* variant_out, void* out, hipStream_t s) {
  const int esz = (int)sizeof(TIN), osz = OUT_BF16 ? 2 : 4;
  const long long rows_need =
      TAPS + ((long long)(kAugBandRows - 1) * max_ch + P.OH - 1) / P.OH;  // TAPS + ⌈(R−1)·ch/OH⌉
  const int rows_cap = (int)(rows_need < max_ch ? rows_need : max_ch);
  const long long pitch_ll = ((long long)max_cw * P.C * esz + 3 + 3) & ~3LL;
  const bool fits = pitch_ll <= kAugLdsBudget && P.OW <= 1024 && ((uintptr_t)src & 3) == 0 &&
                    ((uintptr_t)out & (osz - 1)) == 0 &&
                    aug_lds(P.OW, P.C, osz, 0, 0).total + (long long)rows_cap * pitch_ll <= kAugLdsBudget;
  if (variant == 1 && !fits) return (int)hipErrorInvalidValue;
  const bool staged = variant == 1 || (variant == 0 && fits);
  if (variant_out) *variant_out = staged ? 1 : 2;
  if (staged) {
    const int pitch = (int)pitch_ll;
    const int bands = (P.OH + kAugBandRows - 1) / kAugBandRows;
    const long long grid = (long long)B * bands;
    if (grid > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const int lds = aug_lds(P.OW, P.C, osz, rows_cap, pitch).total;
    hipLaunchKernelGGL((k_img_aug_lds<TIN, TAPS, OUT_BF16>), dim3((unsigned)grid), dim3(kAugThreads), lds, s,
                       (const uint8_t*)src, src_bytes, desc, bands, P, rows_cap, pitch, out);
  } else {
    const int grid = bigdl_grid((long long)B * P.OH * P.OW, kAugThreads, 16384);
    hipLaunchKernelGGL((k_img_aug_direct<TIN, TAPS, OUT_BF16>), dim3(grid), dim3(kAugThreads), 0, s,
                       (const uint8_t*)src, desc, B, P, out);
  }
  BIGDL_CHECK_LAUNCH();
}

}  // namespace

// `desc` is a device table of B rows {byte offset, H, W, y0, x0, ch, cw, flip}; the caller has checked on the
// host that every rectangle lies inside its image and every image inside the `src_bytes` of `src`.
// `max_ch` / `max_cw`: the tallest / widest rectangle of the batch (sizes the staged variant).
// `interp`: 1 LINEAR, 2 CUBIC.  `variant`: 0 pick, 1 staged (an error when it does not fit), 2 direct;
// the variant launched is written to `*variant_out` when given.
BIGDL_EXPORT int bigdl_image_resample_norm(const void* src, long long src_bytes, int src_u8, const long long* desc,
                                           int B, int C, int max_ch, int max_cw, int OH, int OW, const float* mean,
                                           const float* stdv, int to_rgb, int interp, void* out, int out_bf16,
                                           int variant, int* variant_out, hipStream_t s) {
  if (!src || !desc || !out || B <= 0 || C <= 0 || C > 4 || OH <= 0 || OW <= 0 || max_ch <= 0 || max_cw <= 0 ||
      (interp != 1 && interp != 2) || variant < 0 || variant > 2)
    return (int)hipErrorInvalidValue;
  AugParams P;
  for (int c = 0; c < 4; ++c) {
    P.mean[c] = c < C ? mean[c] : 0.f;
    P.inv_std[c] = c < C ? 1.f / stdv[c] : 1.f;
  }
  P.C = C;
  P.OH = OH;
  P.OW = OW;
  P.to_rgb = to_rgb;
#define AUG_GO(TIN, TAPS, BF) \
  return aug_launch<TIN, TAPS, BF>(src, src_bytes, desc, B, P, max_ch, max_cw, variant, variant_out, out, s)
  if (src_u8) {
    if (interp == 2) {
      if (out_bf16) AUG_GO(uint8_t, 4, true);
      AUG_GO(uint8_t, 4, false);
    }
    if (out_bf16) AUG_GO(uint8_t, 2, true);
    AUG_GO(uint8_t, 2, false);
  }
  if (interp == 2) {
    if (out_bf16) AUG_GO(float, 4, true);
    AUG_GO(float, 4, false);
  }
  if (out_bf16) AUG_GO(float, 2, true);
  AUG_GO(float, 2, false);
#undef AUG_GO
}
