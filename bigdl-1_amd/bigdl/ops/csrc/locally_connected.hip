// LocallyConnected2D / LocallyConnected1D (nn/layers/conv.py) on the bf16 MFMA: forward, data gradient and
// weight gradient of a convolution whose every output location l has its own filter W[l] = [O][K],
// K = C·T (T = kH·kW taps).  Each weight is used N times per pass (N = batch), so the forward and the data
// gradient are bound by reading the weights and the weight gradient by its fp32 store: every pass touches a
// weight byte once, where the layer keeps it, and nothing of the size of a column tensor is ever built.
//
//   y[n,l,o]  = bias[l,o] + Σ_k W[l,o,k] · P_l[n,k]           k_lc_gemm  (P_l: the input patch of location l)
//   gx[n,p,c] = Σ_(slot,o) Wd[p,c,slot,o] · gy[n,l(p,slot),o]  k_lc_wt, then k_lc_gemm<TC> over input pixels p
//   gW[l,o,k] = s · Σ_n gy[n,l,o] · P_l[n,k]                   k_lc_wgrad
//
// Reduction orders.  The 2-D layer's K runs (c, ky, kx) ("CT"), the 1-D layer's (kx, c) ("TC"), which is NHWC's
// own order.  An MFMA lane wants 8 consecutive reduction elements: a 16-byte read of a weight row as it lies
// gives that, so the weights are never repacked for the forward and it is the small, reused operand, the
// patch, that is rearranged on its way into LDS: TC copies 16-byte global loads as 16-byte LDS stores (a tap
// is C contiguous channels), CT scatters each 16-byte load (8 channels of one tap) as eight 2-byte stores T
// elements apart.  Taps outside the image store zeros.
//
// k_lc_gemm.  A block of 4 waves owns one location, 64 batch rows (the batch tile is the grid's fastest index:
// the other tiles of a location find its weights in L2) and 64 output channels; the waves split the output
// channels, 16 each, so a wave holds 4 accumulator tiles (16 VGPRs) and no fold through LDS is needed (a
// split over K would hold 16 tiles per wave and fold them).  The patch tile [64][128 of K] goes through a
// two-stage LDS ring, staged once per block for all four waves; its row pitch is 17 sixteen-byte units
// (odd), so the 16 row lanes of a ds_read_b128 fragment fall on different slots.  The weight fragments go
// from global memory straight to registers, the four k-steps of a 128-column chunk issued together one
// chunk ahead (a row's loads then cover 256 contiguous bytes).  The epilogue adds the fp32 bias row and
// stores bf16; rows ≥ N and channels ≥ O are masked.
//
// Data gradient.  For an input pixel p the gradient is again a per-location product whose reduction
// (slot, o) lies in gy's NHWC order; a slot enumerates the ⌈kH/sH⌉·⌈kW/sW⌉ taps that can reach p.  k_lc_wt
// writes Wd[p][c][slot][o] = W[l(p,slot)][o][c][tap] (a block reads a [64 o][128 k] piece of a location's
// slab coalesced into LDS and writes O-contiguous 16-byte segments; slots no location reaches stay zero),
// then the TC body gathers gy "patches".  No atomics, no column buffer; one extra read and write of the
// weights per backward, cached by the caller per weight generation.
//
// k_lc_wgrad.  A block owns a location, 64 output channels and 128 of K and loops over ALL batch rows in
// stages of 32 (zero-filled beyond N), so every gW element is written exactly once: no split-K, no atomics.
// The reduction index n is the strided dimension of both operands: the gy tile [n][o] and the patch tile
// [n][k] lie row-major in LDS (same staging as above) and the fragments are read transposed
// (ds_read_b64_tr_b16).  The waves split the 128 K columns, 32 each, and store fp32 along k.
#include "common.h"

typedef short v8s __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lc_lds_v4s;

constexpr int kLcRows = 64;               // batch rows of a gemm block
constexpr int kLcKc = 128;                // reduction columns staged at a time
constexpr int kLcPitch = kLcKc / 8 + 1;   // patch tile row pitch, 16-byte units (odd)
constexpr int kLcOt = 64;                 // output channels of a block
constexpr int kLcGyPitch = kLcOt / 8 + 1;  // gy tile row pitch (wgrad), 16-byte units
constexpr int kLcWgRows = 32;             // batch rows of a wgrad stage: one MFMA k-step
constexpr int kLcMaxT = 256;              // taps (or slots) a block tabulates
constexpr int kLcWtPitch = kLcOt + 8;     // k_lc_wt LDS row pitch, elements (9 sixteen-byte units)

enum { LC_CT = 0, LC_TC = 1 };

// The layer's geometry: input image H×W×C, window kH×kW, output grid oH×oW×O.
struct LcGeom {
  int H, W, C, O, kH, kW, sH, sW, pH, pW, oH, oW;
};

struct LcP {
  const bf16_t* src;   // gather source [N][srcHW][Cs]: the input image, or gy for the data gradient
  const bf16_t* w;     // [L][Oc][K]
  const float* bias;   // [L][Oc] or null
  bf16_t* y;           // [N][L][Oc]
  int N, Cs, T, K, Oc, L, srcHW;
  int slots;           // 0: tap t is window element (ky, kx) of output location l; 1: slot t of input pixel l
  LcGeom g;
};

// Source pixel of tap (slot) t of location loc, or −1 where there is none.
__device__ __forceinline__ int lc_tap_pixel(const LcGeom& g, int slots, int loc, int t) {
  if (!slots) {
    const int oy = loc / g.oW, ox = loc - oy * g.oW, ky = t / g.kW, kx = t - ky * g.kW;
    const int iy = oy * g.sH - g.pH + ky, ix = ox * g.sW - g.pW + kx;
    return (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) ? iy * g.W + ix : -1;
  }
  const int sb = (g.kW + g.sW - 1) / g.sW;
  const int iy = loc / g.W, ix = loc - iy * g.W, a = t / sb, b = t - a * sb;
  const int ky = (iy + g.pH) % g.sH + a * g.sH, kx = (ix + g.pW) % g.sW + b * g.sW;
  const int dy = iy + g.pH - ky, dx = ix + g.pW - kx;
  if (ky >= g.kH || kx >= g.kW || dy < 0 || dx < 0) return -1;
  const int oy = dy / g.sH, ox = dx / g.sW;
  return (oy < g.oH && ox < g.oW) ? oy * g.oW + ox : -1;
}

// Stage rows [n0, n0 + rows) × reduction columns [k0, k0 + len) of the patch matrix into an LDS tile
// (row pitch in 16-byte units).  len is a multiple of 8 and at most kLcKc.
template <int ORDER>
__device__ __forceinline__ void lc_stage(bigdl_u32x4* tile, int pitch, const bf16_t* __restrict__ src, const int* s_pix,
                                         int N, int Cs, int T, int srcHW, int n0, int rows, int k0, int len, int tid) {
  const bigdl_u32x4 zero = {0u, 0u, 0u, 0u};
  if constexpr (ORDER == LC_TC) {
    const int nu = ((len + 31) >> 5) << 2;   // whole k-steps: the tail is zero
    for (int idx = tid; idx < rows * nu; idx += 256) {
      const int row = idx / nu, u = idx - row * nu, k = k0 + u * 8, n = n0 + row;
      bigdl_u32x4 v = zero;
      if (n < N && u * 8 < len) {
        const int t = k / Cs, c = k - t * Cs, pix = s_pix[t];
        if (pix >= 0) v = *reinterpret_cast<const bigdl_u32x4*>(src + ((long long)n * srcHW + pix) * Cs + c);
      }
      tile[row * pitch + u] = v;
    }
  } else {
    // the 8-channel groups that hold a channel of this chunk, every tap of each
    const int g_lo = (k0 / T) >> 3, ng = (((k0 + len - 1) / T) >> 3) - g_lo + 1, per = T * ng;
    bf16_t* t16 = reinterpret_cast<bf16_t*>(tile);
    for (int idx = tid; idx < rows * per; idx += 256) {
      const int row = idx / per, r = idx - row * per, t = r / ng, gch = (g_lo + r - t * ng) * 8, n = n0 + row;
      const int pix = s_pix[t];
      bigdl_u32x4 v = zero;
      if (n < N && pix >= 0) v = *reinterpret_cast<const bigdl_u32x4*>(src + ((long long)n * srcHW + pix) * Cs + gch);
      bf16_t* dst = t16 + row * pitch * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = (gch + j) * T + t - k0;
        if ((unsigned)k < (unsigned)len) dst[k] = (bf16_t)(v[j >> 1] >> ((j & 1) * 16));
      }
    }
  }
}

template <int ORDER>
__global__ void __launch_bounds__(256) k_lc_gemm(LcP p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 lds[2][kLcRows * kLcPitch];
  __shared__ int s_pix[kLcMaxT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * kLcRows, l = blockIdx.y, ob = blockIdx.z * kLcOt + wid * 16;
  const int K = p.K;

  for (int t = tid; t < p.T; t += 256) s_pix[t] = lc_tap_pixel(p.g, p.slots, l, t);
  // columns between a chunk's end and its last k-step must hold finite values (their weights read as zero)
  for (int idx = tid; idx < 2 * kLcRows * kLcPitch; idx += 256) (&lds[0][0])[idx] = bigdl_u32x4{0u, 0u, 0u, 0u};
  __syncthreads();

  const int o = ob + fr;
  const bool w_on = o < p.Oc;   // false for a whole wave when its 16 channels lie beyond O
  const bf16_t* wrow = p.w + ((long long)l * p.Oc + (w_on ? o : 0)) * K;
  const int nq = min(4, (p.N - n0 + 15) >> 4);   // 16-row fragments that hold a row < N
  const int nch = (K + kLcKc - 1) / kLcKc;

  v4f acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = v4f{0.f, 0.f, 0.f, 0.f};

  bigdl_u32x4 wv[4], wn[4];
  auto load_w = [&](int k0, bigdl_u32x4(&dst)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + s * 32 + fq * 8;
      dst[s] = (w_on && k < K) ? *reinterpret_cast<const bigdl_u32x4*>(wrow + k) : bigdl_u32x4{0u, 0u, 0u, 0u};
    }
  };

  load_w(0, wv);
  lc_stage<ORDER>(lds[0], kLcPitch, p.src, s_pix, p.N, p.Cs, p.T, p.srcHW, n0, kLcRows, 0, min(kLcKc, K), tid);
  __syncthreads();
  for (int i = 0; i < nch; ++i) {
    const int buf = i & 1, k0 = i * kLcKc;
    if (i + 1 < nch) {
      load_w(k0 + kLcKc, wn);
      lc_stage<ORDER>(lds[buf ^ 1], kLcPitch, p.src, s_pix, p.N, p.Cs, p.T, p.srcHW, n0, kLcRows, k0 + kLcKc,
                      min(kLcKc, K - k0 - kLcKc), tid);
    }
    if (ob < p.Oc) {
      const int nks = (min(kLcKc, K - k0) + 31) >> 5;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < nks) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (q < nq) {
              const v8s xf = __builtin_bit_cast(v8s, lds[buf][(q * 16 + fr) * kLcPitch + s * 4 + fq]);
              acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8s, wv[s]), xf, acc[q], 0, 0, 0);
            }
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) wv[s] = wn[s];
    __syncthreads();
  }

  // accumulator element e of lane (fr, fq): row n0 + 16q + fr, channels ob + 4fq + e
  const int o4 = ob + fq * 4;
  if (o4 >= p.Oc) return;
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) {
    const float4 bv = *reinterpret_cast<const float4*>(p.bias + (long long)l * p.Oc + o4);
    b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + q * 16 + fr;
    if (n >= p.N) continue;
    const uint32_t lo = (uint32_t)f2bf(acc[q][0] + b[0]) | ((uint32_t)f2bf(acc[q][1] + b[1]) << 16);
    const uint32_t hi = (uint32_t)f2bf(acc[q][2] + b[2]) | ((uint32_t)f2bf(acc[q][3] + b[3]) << 16);
    *reinterpret_cast<uint2*>(p.y + ((long long)n * p.L + l) * p.Oc + o4) = make_uint2(lo, hi);
  }
}

// ------------------------------------------------------------------------------------------------
// Wd[p][c][slot][o] = W[l][o][k(c, tap)] for the input pixel p and slot that tap (ky, kx) of location l reaches.
// Wd is cleared first: (p, slot) pairs no location reaches stay zero.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lc_fill0(bigdl_u32x4* __restrict__ dst, long long n) {
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < n; idx += gridDim.x * 256LL)
    dst[idx] = bigdl_u32x4{0u, 0u, 0u, 0u};
}

template <int ORDER>
__global__ void __launch_bounds__(256) k_lc_wt(const bf16_t* __restrict__ w, bf16_t* __restrict__ wd, LcGeom g) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[kLcKc * kLcWtPitch];
  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * kLcKc, ob = blockIdx.y * kLcOt, l = blockIdx.z;
  const int T = g.kH * g.kW, K = g.C * T, O = g.O;
  const int sa = (g.kH + g.sH - 1) / g.sH, sb = (g.kW + g.sW - 1) / g.sW, S = sa * sb;
  for (int idx = tid; idx < kLcOt * (kLcKc / 8); idx += 256) {
    const int orow = idx >> 4, u = idx & 15, o = ob + orow, k = k0 + u * 8;
    bigdl_u32x4 v = {0u, 0u, 0u, 0u};
    if (o < O && k < K) v = *reinterpret_cast<const bigdl_u32x4*>(w + ((long long)l * O + o) * K + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[(u * 8 + j) * kLcWtPitch + orow] = (bf16_t)(v[j >> 1] >> ((j & 1) * 16));
  }
  __syncthreads();
  const int oy = l / g.oW, ox = l - oy * g.oW;
  for (int idx = tid; idx < kLcKc * (kLcOt / 8); idx += 256) {
    const int kk = idx >> 3, og = idx & 7, k = k0 + kk, o = ob + og * 8;
    if (k >= K || o >= O) continue;
    int c, t;
    if constexpr (ORDER == LC_CT) { c = k / T; t = k - c * T; }
    else { t = k / g.C; c = k - t * g.C; }
    const int ky = t / g.kW, kx = t - ky * g.kW;
    const int iy = oy * g.sH - g.pH + ky, ix = ox * g.sW - g.pW + kx;
    if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
    const int slot = (ky / g.sH) * sb + kx / g.sW;
    *reinterpret_cast<bigdl_u32x4*>(wd + (((long long)(iy * g.W + ix) * g.C + c) * S + slot) * O + o) =
        *reinterpret_cast<const bigdl_u32x4*>(tile + kk * kLcWtPitch + og * 8);
  }
}

// ------------------------------------------------------------------------------------------------
// gW[l][o][k] = scale · Σ_n gy[n][l][o] · P_l[n][k]
// ------------------------------------------------------------------------------------------------
struct LcW {
  const bf16_t* x;    // [N][H·W][C]
  const bf16_t* gy;   // [N][L][O]
  float* gw;          // [L][O][K]
  float scale;
  int N, T, K, L;
  LcGeom g;
};

template <int ORDER>
__global__ void __launch_bounds__(256) k_lc_wgrad(LcW p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_gy[2][kLcWgRows * kLcGyPitch];
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_pt[2][kLcWgRows * kLcPitch];
  __shared__ int s_pix[kLcMaxT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int k0 = blockIdx.x * kLcKc, ob = blockIdx.y * kLcOt, l = blockIdx.z;
  const int K = p.K, O = p.g.O, len = min(kLcKc, K - k0);

  for (int t = tid; t < p.T; t += 256) s_pix[t] = lc_tap_pixel(p.g, 0, l, t);
  __syncthreads();

  auto stage = [&](int buf, int n0) {
    {  // gy tile [32][64]: one 16-byte unit per thread
      const int row = tid >> 3, u = tid & 7, n = n0 + row, o = ob + u * 8;
      bigdl_u32x4 v = {0u, 0u, 0u, 0u};
      if (n < p.N && o < O) v = *reinterpret_cast<const bigdl_u32x4*>(p.gy + ((long long)n * p.L + l) * O + o);
      s_gy[buf][row * kLcGyPitch + u] = v;
    }
    lc_stage<ORDER>(s_pt[buf], kLcPitch, p.x, s_pix, p.N, p.g.C, p.T, p.g.H * p.g.W, n0, kLcWgRows, k0, len, tid);
  };

  v4f acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  // transposed fragment: lane 4q + p of a 16-lane group addresses row r0 + q, columns col + 4p .. + 3 and
  // receives column col + (lane & 15) of rows r0 .. r0 + 3; the group fq holds stage rows 8fq .. 8fq + 7
  const int trow = 8 * fq + (fr >> 2), tcol = 4 * (fr & 3);
  auto frag = [&](const bigdl_u32x4* tile, int pitch, int col) -> v8s {
    const bf16_t* base = reinterpret_cast<const bf16_t*>(tile) + trow * pitch * 8 + col + tcol;
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lc_lds_v4s*)base);
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lc_lds_v4s*)(base + 4 * pitch * 8));
    return v8s{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };

  const int nst = (p.N + kLcWgRows - 1) / kLcWgRows;
  const int kw = wid * 32;   // this wave's 32 columns of the chunk
  stage(0, 0);
  __syncthreads();
  for (int i = 0; i < nst; ++i) {
    const int buf = i & 1;
    if (i + 1 < nst) stage(buf ^ 1, (i + 1) * kLcWgRows);
    if (kw < len) {
      v8s bfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = frag(s_pt[buf], kLcPitch, kw + j * 16);
#pragma unroll
      for (int oi = 0; oi < 4; ++oi) {
        if (ob + oi * 16 < O) {
          const v8s af = frag(s_gy[buf], kLcGyPitch, oi * 16);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[oi][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[j], acc[oi][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // accumulator element e of lane (fr, fq): channel ob + 16oi + 4fq + e, column k0 + kw + 16j + fr
#pragma unroll
  for (int oi = 0; oi < 4; ++oi)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + kw + j * 16 + fr;
      if (k >= K) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int o = ob + oi * 16 + fq * 4 + e;
        if (o < O) p.gw[((long long)l * O + o) * K + k] = p.scale * acc[oi][j][e];
      }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static bool lc_geom(LcGeom& g, int H, int W, int C, int O, int kH, int kW, int sH, int sW, int pH, int pW) {
  if (H <= 0 || W <= 0 || C <= 0 || O <= 0 || kH <= 0 || kW <= 0 || sH <= 0 || sW <= 0 || pH < 0 || pW < 0) return false;
  if (C % 8 || O % 8 || H + 2 * pH < kH || W + 2 * pW < kW) return false;
  g = LcGeom{H, W, C, O, kH, kW, sH, sW, pH, pW, (H + 2 * pH - kH) / sH + 1, (W + 2 * pW - kW) / sW + 1};
  const long long T = (long long)kH * kW, L = (long long)g.oH * g.oW, P = (long long)H * W;
  // a block tabulates its taps; locations and pixels are grid.y / grid.z; K and per-image sizes stay in int
  return T <= kLcMaxT && L <= 65535 && P <= 65535 && T * C < (1 << 24) && T * O < (1 << 24) && P * C < (1LL << 31) &&
         L * O < (1LL << 31);
}

static int lc_slots(const LcGeom& g) { return ((g.kH + g.sH - 1) / g.sH) * ((g.kW + g.sW - 1) / g.sW); }

static inline bool lc_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

static int lc_gemm_launch(int order, const LcP& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.N + kLcRows - 1) / kLcRows), (unsigned)p.L, (unsigned)((p.Oc + kLcOt - 1) / kLcOt)), blk(256);
  if (grid.z > 65535) return (int)hipErrorInvalidValue;
  if (order == LC_CT) hipLaunchKernelGGL(k_lc_gemm<LC_CT>, grid, blk, 0, s, p);
  else hipLaunchKernelGGL(k_lc_gemm<LC_TC>, grid, blk, 0, s, p);
  return (int)hipGetLastError();
}

// y [N][L][O] bf16 = per-location product of x [N][H][W][C] bf16 and w [L][O][K] bf16 (+ fp32 bias [L][O]).
BIGDL_EXPORT int bigdl_lc_forward(int order, const void* x, const void* w, const float* bias, void* y, int N, int H, int W,
                                  int C, int O, int kH, int kW, int sH, int sW, int pH, int pW, hipStream_t s) {
  LcGeom g;
  if ((order != LC_CT && order != LC_TC) || N <= 0 || !x || !w || !y || !lc_geom(g, H, W, C, O, kH, kW, sH, sW, pH, pW) ||
      !lc_al16(x) || !lc_al16(w) || !lc_al16(y) || !lc_al16(bias))
    return (int)hipErrorInvalidValue;
  LcP p{};
  p.src = (const bf16_t*)x; p.w = (const bf16_t*)w; p.bias = bias; p.y = (bf16_t*)y;
  p.N = N; p.Cs = C; p.T = kH * kW; p.K = C * p.T; p.Oc = O; p.L = g.oH * g.oW; p.srcHW = H * W; p.slots = 0; p.g = g;
  return lc_gemm_launch(order, p, s);
}

// Elements of the transposed weights Wd [H·W][C][slots][O] of a geometry (0: not taken).
BIGDL_EXPORT long long bigdl_lc_wd_numel(int H, int W, int C, int O, int kH, int kW, int sH, int sW, int pH, int pW) {
  LcGeom g;
  if (!lc_geom(g, H, W, C, O, kH, kW, sH, sW, pH, pW) || lc_slots(g) > kLcMaxT) return 0;
  return (long long)H * W * C * lc_slots(g) * O;
}

BIGDL_EXPORT int bigdl_lc_weight_transpose(int order, const void* w, void* wd, int H, int W, int C, int O, int kH, int kW,
                                           int sH, int sW, int pH, int pW, hipStream_t s) {
  const long long n = bigdl_lc_wd_numel(H, W, C, O, kH, kW, sH, sW, pH, pW);
  LcGeom g;
  if ((order != LC_CT && order != LC_TC) || n <= 0 || !w || !wd || !lc_al16(w) || !lc_al16(wd) ||
      !lc_geom(g, H, W, C, O, kH, kW, sH, sW, pH, pW))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lc_fill0, dim3(bigdl_grid(n / 8, 256)), dim3(256), 0, s, (bigdl_u32x4*)wd, n / 8);
  const int K = C * kH * kW;
  const dim3 grid((unsigned)((K + kLcKc - 1) / kLcKc), (unsigned)((O + kLcOt - 1) / kLcOt), (unsigned)(g.oH * g.oW));
  if (order == LC_CT) hipLaunchKernelGGL(k_lc_wt<LC_CT>, grid, dim3(256), 0, s, (const bf16_t*)w, (bf16_t*)wd, g);
  else hipLaunchKernelGGL(k_lc_wt<LC_TC>, grid, dim3(256), 0, s, (const bf16_t*)w, (bf16_t*)wd, g);
  return (int)hipGetLastError();
}

// gx [N][H][W][C] bf16 from gy [N][L][O] bf16 and the transposed weights Wd.
BIGDL_EXPORT int bigdl_lc_dgrad(const void* gy, const void* wd, void* gx, int N, int H, int W, int C, int O, int kH, int kW,
                                int sH, int sW, int pH, int pW, hipStream_t s) {
  LcGeom g;
  if (N <= 0 || !gy || !wd || !gx || !lc_geom(g, H, W, C, O, kH, kW, sH, sW, pH, pW) || lc_slots(g) > kLcMaxT ||
      !lc_al16(gy) || !lc_al16(wd) || !lc_al16(gx))
    return (int)hipErrorInvalidValue;
  LcP p{};
  p.src = (const bf16_t*)gy; p.w = (const bf16_t*)wd; p.bias = nullptr; p.y = (bf16_t*)gx;
  p.N = N; p.Cs = O; p.T = lc_slots(g); p.K = O * p.T; p.Oc = C; p.L = H * W; p.srcHW = g.oH * g.oW; p.slots = 1; p.g = g;
  return lc_gemm_launch(LC_TC, p, s);
}

// gw [L][O][K] fp32 = scale · the weight gradient (every element written once).
BIGDL_EXPORT int bigdl_lc_wgrad(int order, const void* x, const void* gy, float* gw, float scale, int N, int H, int W,
                                int C, int O, int kH, int kW, int sH, int sW, int pH, int pW, hipStream_t s) {
  LcGeom g;
  if ((order != LC_CT && order != LC_TC) || N <= 0 || !x || !gy || !gw || !lc_geom(g, H, W, C, O, kH, kW, sH, sW, pH, pW) ||
      !lc_al16(x) || !lc_al16(gy))
    return (int)hipErrorInvalidValue;
  LcW p{};
  p.x = (const bf16_t*)x; p.gy = (const bf16_t*)gy; p.gw = gw; p.scale = scale;
  p.N = N; p.T = kH * kW; p.K = C * p.T; p.L = g.oH * g.oW; p.g = g;
  const dim3 grid((unsigned)((p.K + kLcKc - 1) / kLcKc), (unsigned)((O + kLcOt - 1) / kLcOt), (unsigned)p.L);
  if (order == LC_CT) hipLaunchKernelGGL(k_lc_wgrad<LC_CT>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(k_lc_wgrad<LC_TC>, grid, dim3(256), 0, s, p);
  return (int)hipGetLastError();
}
