// Bilinear (nn/layers/linear.py) on the bf16 MFMA: y[b,k] = x1[b,:]ᵀ · W[k] · x2[b,:] + bias[k] and its three
// gradients.  Every pass is a GEMM (2·B·K·I·J flops) with a small reduction or scaling on its accumulators;
// none of them writes a [B][K][I] or [B][K][J] intermediate to global memory, and W [K][I][J] is read where the
// layer keeps it (the arena's bf16 shadow), never transposed or repacked.
//
//   y[b,k]    = bias[k] + Σ_i x1[b,i] · U_k[b,i]     U_k[b,i] = Σ_j x2[b,j] · W[k,i,j]     k_bil_u<BIL_FWD>
//   gx1[b,i]  = Σ_k gy[b,k] · U_k[b,i]                                                      k_bil_u<BIL_GX1>
//   gx2[b,j]  = Σ_k gy[b,k] · V_k[b,j]               V_k[b,j] = Σ_i x1[b,i] · W[k,i,j]     k_bil_v
//   gW[k,i,j] = s · Σ_b (gy[b,k] · x1[b,i]) · x2[b,j]                                       k_bil_wgrad
//
// k_bil_u.  U_k reduces over j, along which W's rows are contiguous: W is the MFMA A operand exactly as it lies,
// read 16 bytes per lane from global memory straight to registers, the four k-steps of a 128-column chunk
// issued together one chunk ahead.  The x2 tile [32 rows][128 of J] goes through a two-stage LDS ring (row pitch
// 17 sixteen-byte units, odd), its global loads issued before the chunk's MFMAs and stored to LDS after them;
// with J ≤ 128 it is staged once.  A wave owns one 16-row slab of one W[k] at a time ("unit") and walks its j
// chunks; when the unit's U tile [32][16] is complete in the accumulators the epilogue runs on them in fp32:
//   forward  a block owns 32 batch rows and one k; the waves take the i slabs 16·(4g + wave); the tile is
//            multiplied by x1[b,i] and summed in-lane into one partial per row fragment.  After the last slab the
//            partials are reduced across the four lane groups (two xor shuffles) and across the waves (one LDS
//            pass); bias is added and y[b,k] written once.
//   gx1      a block owns 32 batch rows and 16 columns of I; the waves take k = 4g + wave (all four share the
//            x2 chunk in LDS) and do out += float(gy[b,k]) · U.  The four waves' tiles are folded through LDS in
//            a fixed order and gx1 is written once.
// k_bil_v.  V_k reduces over i, W's strided dimension.  A block owns 32 batch rows and 64 columns of J (16 per
// wave) and loops k; W_k[64 of I][64 of J] is staged in LDS as it lies and the A fragments are read transposed
// (ds_read_b64_tr_b16); x1's tile [32][64 of I] is staged beside it.  out += float(gy[b,k]) · V in registers,
// gx2 written once.  (A kernel of its own, not a flag of k_bil_u: the operand paths differ, only the
// epilogue is shared.)
// k_bil_wgrad.  A block owns one k, 64 rows of I and 128 columns of J (32 per wave) and sums ALL batch rows in
// stages of 32: each gW element is written once, no split, no atomics.  Both operands are batch-strided, so both
// fragments are transposed LDS reads.  The A operand is the product p = gy[b,k]·x1[b,i]: two bf16 factors give
// at most 16 significant bits, so hi = bf16(p), lo = bf16(p − hi) hold p exactly, and two MFMAs per step sum the
// exact products in fp32 (one bf16 rounding of p would cost 2⁻⁹ per term).  The block of the first I and J tile
// also sums its column of gy, which it loads anyway: the bias gradient, for any K (the column-sum kernel
// takes only multiples of 8).
//
// Tails in B, I, J and any K ≥ 1 are zero-filled on load and masked on store; I and J must be multiples of 8.
// Every result is the same bits on every run.
#include "common.h"

typedef short v8s __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s bil_lds_v4s;

constexpr int kBilRows = 32;                // batch rows of a block: two MFMA row fragments
constexpr int kBilNq = kBilRows / 16;
constexpr int kBilJc = 128;                 // k_bil_u: columns of J staged at a time
constexpr int kBilPitch = kBilJc / 8 + 1;   // x2 tile row pitch, 16-byte units (odd)
constexpr int kBilIc = 64;                  // k_bil_v: rows of I staged at a time; k_bil_wgrad: its I tile
constexpr int kBilJt = 64;                  // k_bil_v: columns of J of a block
constexpr int kBilPitch64 = 64 / 8 + 1;     // row pitch of a 64-column tile, 16-byte units

enum { BIL_FWD = 0, BIL_GX1 = 1 };

struct BilP {
  const bf16_t* x1;    // [B][I]   (forward, gx2, wgrad)
  const bf16_t* x2;    // [B][J]   (forward, gx1, wgrad)
  const bf16_t* w;     // [K][I][J]
  const bf16_t* gy;    // [B][K]   (gradients)
  const float* bias;   // [K] or null (forward)
  bf16_t* out;         // y [B][K], gx1 [B][I] or gx2 [B][J]
  int B, I, J, K;
};

__device__ __forceinline__ bigdl_u32x4 bil_ld16(const bf16_t* p, bool on) {
  return on ? *reinterpret_cast<const bigdl_u32x4*>(p) : bigdl_u32x4{0u, 0u, 0u, 0u};
}

// Transposed fragment of a row-major bf16 LDS tile (pitch in 16-byte units): lane (fr, fq) receives column
// col + fr of rows r0 + 8fq .. r0 + 8fq + 7.  Lane 4q + p of a 16-lane group addresses row r0 + 8fq + q, columns
// col + 4p .. + 3.
__device__ __forceinline__ v8s bil_frag_t(const bigdl_u32x4* tile, int pitch, int r0, int col, int fr, int fq) {
  const bf16_t* base = reinterpret_cast<const bf16_t*>(tile) + (r0 + 8 * fq + (fr >> 2)) * pitch * 8 + col + 4 * (fr & 3);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bil_lds_v4s*)base);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bil_lds_v4s*)(base + 4 * pitch * 8));
  return v8s{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// bf16 store of accumulator tiles: element e of lane (fr, fq) of fragment q is row n0 + 16q + fr, column c0 + 4fq + e
__device__ __forceinline__ void bil_store_tile(bf16_t* out, const v4f (&t)[kBilNq], int n0, int B, int c0, int C, int fr, int fq) {
  const int c = c0 + fq * 4;
  if (c >= C) return;
#pragma unroll
  for (int q = 0; q < kBilNq; ++q) {
    const int n = n0 + q * 16 + fr;
    if (n >= B) continue;
    const uint32_t lo = (uint32_t)f2bf(t[q][0]) | ((uint32_t)f2bf(t[q][1]) << 16);
    const uint32_t hi = (uint32_t)f2bf(t[q][2]) | ((uint32_t)f2bf(t[q][3]) << 16);
    *reinterpret_cast<uint2*>(out + (long long)n * C + c) = make_uint2(lo, hi);
  }
}

// ------------------------------------------------------------------------------------------------
// forward and gx1: the reduction runs along W's rows
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256) k_bil_u(BilP p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 lds[2][kBilRows * kBilPitch];
  __shared__ float s_red[4][kBilRows];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * kBilRows;
  const int B = p.B, I = p.I, J = p.J, K = p.K;
  const int nch = (J + kBilJc - 1) / kBilJc;                                   // j chunks of a unit
  const int units = MODE == BIL_FWD ? ((I + 15) / 16 + 3) / 4 : (K + 3) / 4;   // units of a wave
  const int steps = units * nch;
  const bool ring = nch > 1;   // with one chunk the x2 tile is staged once and stays in lds[0]

  // the W row of this lane in unit g: forward k = blockIdx.y, i slab 4g + wave; gx1 k = 4g + wave
  bigdl_u32x4 wv[4], wn[4];
  auto load_w = [&](int step, bigdl_u32x4(&dst)[4]) {
    const int g = step / nch, j0 = (step - g * nch) * kBilJc + fq * 8;
    const int k = MODE == BIL_FWD ? (int)blockIdx.y : g * 4 + wid;
    const int i = (MODE == BIL_FWD ? (g * 4 + wid) * 16 : (int)blockIdx.y * 16) + fr;
    const bool on = k < K && i < I;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = j0 + s * 32;
      dst[s] = (on && j < J) ? *reinterpret_cast<const bigdl_u32x4*>(p.w + ((long long)k * I + i) * J + j)
                             : bigdl_u32x4{0u, 0u, 0u, 0u};
    }
  };
  // the x2 tile of chunk c: one 16-byte unit per thread and pass, rows ≥ B and columns ≥ J zero
  bigdl_u32x4 xs[kBilRows * (kBilJc / 8) / 256];
  auto load_x = [&](int c) {
#pragma unroll
    for (int r = 0; r < kBilRows * (kBilJc / 8) / 256; ++r) {
      const int idx = r * 256 + tid, row = idx >> 4, j = c * kBilJc + (idx & 15) * 8, n = n0 + row;
      xs[r] = bil_ld16(p.x2 + (long long)n * J + j, n < B && j < J);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int r = 0; r < kBilRows * (kBilJc / 8) / 256; ++r) {
      const int idx = r * 256 + tid;
      lds[buf][(idx >> 4) * kBilPitch + (idx & 15)] = xs[r];
    }
  };

  v4f acc[kBilNq], out[kBilNq];   // out: gx1's tile; forward keeps its per-row partial in out[q][0]
#pragma unroll
  for (int q = 0; q < kBilNq; ++q) acc[q] = out[q] = v4f{0.f, 0.f, 0.f, 0.f};

  load_w(0, wv);
  load_x(0);
  store_x(0);
  __syncthreads();
  for (int st = 0; st < steps; ++st) {
    const int g = st / nch, c = st - g * nch, buf = ring ? (st & 1) : 0;
    const bool more = st + 1 < steps;
    if (more) {
      load_w(st + 1, wn);
      if (ring) load_x((st + 1) % nch);
    }
    const int nks = (min(kBilJc, J - c * kBilJc) + 31) >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < nks) {
#pragma unroll
        for (int q = 0; q < kBilNq; ++q) {
          const v8s xf = __builtin_bit_cast(v8s, lds[buf][(q * 16 + fr) * kBilPitch + s * 4 + fq]);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8s, wv[s]), xf, acc[q], 0, 0, 0);
        }
      }
    }
    if (c == nch - 1) {
      // U of unit g is complete: element e of lane (fr, fq) of fragment q is row n0 + 16q + fr, W row 4fq + e
#pragma unroll
      for (int q = 0; q < kBilNq; ++q) {
        const int n = n0 + q * 16 + fr;
        if constexpr (MODE == BIL_FWD) {
          const int i = (g * 4 + wid) * 16 + fq * 4;
          if (n < B && i < I) {
            const uint2 xv = *reinterpret_cast<const uint2*>(p.x1 + (long long)n * I + i);
            out[q][0] += acc[q][0] * __uint_as_float(xv.x << 16) + acc[q][1] * __uint_as_float(xv.x & 0xFFFF0000u) +
                         acc[q][2] * __uint_as_float(xv.y << 16) + acc[q][3] * __uint_as_float(xv.y & 0xFFFF0000u);
          }
        } else {
          const int k = g * 4 + wid;
          const float gv = (n < B && k < K) ? bf2f(p.gy[(long long)n * K + k]) : 0.f;
          out[q] += gv * acc[q];
        }
        acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < 4; ++s) wv[s] = wn[s];
      if (ring) {
        store_x(buf ^ 1);
        __syncthreads();
      }
    }
  }

  if constexpr (MODE == BIL_FWD) {
#pragma unroll
    for (int q = 0; q < kBilNq; ++q) {
      float v = out[q][0];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (fq == 0) s_red[wid][q * 16 + fr] = v;
    }
    __syncthreads();
    if (tid < kBilRows && n0 + tid < B) {
      const float v = ((s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid])) + (p.bias ? p.bias[blockIdx.y] : 0.f);
      p.out[(long long)(n0 + tid) * K + blockIdx.y] = f2bf(v);
    }
  } else {
    // fold the four waves' tiles (their k's) in a fixed order; the ring is free after the barrier
    __syncthreads();
    v4f* fold = reinterpret_cast<v4f*>(&lds[0][0]);   // [wave][fragment][lane]: 4·2·64·16 B = 8 KB of the 17 KB
#pragma unroll
    for (int q = 0; q < kBilNq; ++q) fold[(wid * kBilNq + q) * 64 + lane] = out[q];
    __syncthreads();
    if (wid == 0) {
      v4f t[kBilNq];
#pragma unroll
      for (int q = 0; q < kBilNq; ++q)
        t[q] = (fold[q * 64 + lane] + fold[(kBilNq + q) * 64 + lane]) +
               (fold[(2 * kBilNq + q) * 64 + lane] + fold[(3 * kBilNq + q) * 64 + lane]);
      bil_store_tile(p.out, t, n0, B, blockIdx.y * 16, I, fr, fq);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// gx2: the reduction runs across W's rows; W_k tiles are read transposed from LDS
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bil_v(BilP p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_w[2][kBilIc * kBilPitch64];     // [64 of I][64 of J]
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_x[2][kBilRows * kBilPitch64];   // [32 rows][64 of I]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * kBilRows, j0 = blockIdx.y * kBilJt;
  const int B = p.B, I = p.I, J = p.J, K = p.K;
  const int nch = (I + kBilIc - 1) / kBilIc, steps = K * nch;

  // a step's tiles: W_k[i0 .. +63][j0 .. +63] (two units per thread) and x1[n0 .. +31][i0 .. +63] (one unit)
  bigdl_u32x4 ws[2], xs;
  auto load = [&](int step) {
    const int k = step / nch, i0 = (step - k * nch) * kBilIc;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int idx = r * 256 + tid, i = i0 + (idx >> 3), j = j0 + (idx & 7) * 8;
      ws[r] = bil_ld16(p.w + ((long long)k * I + i) * J + j, i < I && j < J);
    }
    const int n = n0 + (tid >> 3), i = i0 + (tid & 7) * 8;
    xs = bil_ld16(p.x1 + (long long)n * I + i, n < B && i < I);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int idx = r * 256 + tid;
      s_w[buf][(idx >> 3) * kBilPitch64 + (idx & 7)] = ws[r];
    }
    s_x[buf][(tid >> 3) * kBilPitch64 + (tid & 7)] = xs;
  };

  v4f acc[kBilNq], out[kBilNq];
#pragma unroll
  for (int q = 0; q < kBilNq; ++q) acc[q] = out[q] = v4f{0.f, 0.f, 0.f, 0.f};

  const bool live = j0 + wid * 16 < J;   // a wave whose 16 columns lie beyond J only helps staging
  load(0);
  store(0);
  __syncthreads();
  for (int st = 0; st < steps; ++st) {
    const int k = st / nch, c = st - k * nch, buf = st & 1;
    const bool more = st + 1 < steps;
    if (more) load(st + 1);
    if (live) {
      const int nks = (min(kBilIc, I - c * kBilIc) + 31) >> 5;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s < nks) {
          const v8s af = bil_frag_t(s_w[buf], kBilPitch64, s * 32, wid * 16, fr, fq);
#pragma unroll
          for (int q = 0; q < kBilNq; ++q) {
            const v8s xf = __builtin_bit_cast(v8s, s_x[buf][(q * 16 + fr) * kBilPitch64 + s * 4 + fq]);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf, acc[q], 0, 0, 0);
          }
        }
      }
      if (c == nch - 1) {
#pragma unroll
        for (int q = 0; q < kBilNq; ++q) {
          const int n = n0 + q * 16 + fr;
          const float gv = n < B ? bf2f(p.gy[(long long)n * K + k]) : 0.f;
          out[q] += gv * acc[q];
          acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    if (more) {
      store(buf ^ 1);
      __syncthreads();
    }
  }
  if (live) bil_store_tile(p.out, out, n0, B, j0 + wid * 16, J, fr, fq);
}

// ------------------------------------------------------------------------------------------------
// gW[k][i][j] = scale · Σ_b (gy[b][k] · x1[b][i]) · x2[b][j]
// ------------------------------------------------------------------------------------------------
struct BilW {
  const bf16_t* x1;
  const bf16_t* x2;
  const bf16_t* gy;
  float* gw;
  float* gb;   // [K] or null: scale · Σ_b gy[b][k], summed by the block of the first I and J tile
  float scale;
  int B, I, J, K;
};

__global__ void __launch_bounds__(256) k_bil_wgrad(BilW p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_hi[2][kBilRows * kBilPitch64];   // [32 rows][64 of I]
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_lo[2][kBilRows * kBilPitch64];
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_x2[2][kBilRows * kBilPitch];     // [32 rows][128 of J]
  __shared__ float s_gb[kBilRows];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int j0 = blockIdx.x * kBilJc, i0 = blockIdx.y * kBilIc, k = blockIdx.z;
  const int B = p.B, I = p.I, J = p.J, K = p.K;

  bigdl_u32x4 x1v, x2v[2];
  float gv, gsum = 0.f;   // gsum: this thread's stage row of gy[:, k] over all stages
  auto load = [&](int b0) {
    const int n = b0 + (tid >> 3), i = i0 + (tid & 7) * 8;
    x1v = bil_ld16(p.x1 + (long long)n * I + i, n < B && i < I);
    gv = n < B ? bf2f(p.gy[(long long)n * K + k]) : 0.f;
    gsum += gv;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int idx = r * 256 + tid, m = b0 + (idx >> 4), j = j0 + (idx & 15) * 8;
      x2v[r] = bil_ld16(p.x2 + (long long)m * J + j, m < B && j < J);
    }
  };
  auto store = [&](int buf) {
    bigdl_u32x4 hi, lo;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      uint32_t hw = 0, lw = 0;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float x = e ? __uint_as_float(x1v[h] & 0xFFFF0000u) : __uint_as_float(x1v[h] << 16);
        // the split is exact for finite operands; an infinite product gives lo = inf − inf = NaN, so gW is NaN
        // where a single rounding would give inf
        const float pr = gv * x;                 // exact: 8 × 8 significant bits
        const bf16_t ph = f2bf(pr);
        const bf16_t pl = f2bf(pr - bf2f(ph));   // exact: what is left has at most 8 significant bits
        hw |= (uint32_t)ph << (16 * e);
        lw |= (uint32_t)pl << (16 * e);
      }
      hi[h] = hw;
      lo[h] = lw;
    }
    s_hi[buf][(tid >> 3) * kBilPitch64 + (tid & 7)] = hi;
    s_lo[buf][(tid >> 3) * kBilPitch64 + (tid & 7)] = lo;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int idx = r * 256 + tid;
      s_x2[buf][(idx >> 4) * kBilPitch + (idx & 15)] = x2v[r];
    }
  };

  v4f acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[a][j] = v4f{0.f, 0.f, 0.f, 0.f};

  const int nst = (B + kBilRows - 1) / kBilRows;
  const int jw = wid * 32;   // this wave's 32 columns of the J tile
  const bool live = j0 + jw < J;
  load(0);
  store(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nst;
    if (more) load((st + 1) * kBilRows);
    if (live) {
      v8s bfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = bil_frag_t(s_x2[buf], kBilPitch, 0, jw + j * 16, fr, fq);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (i0 + a * 16 < I) {
          const v8s ah = bil_frag_t(s_hi[buf], kBilPitch64, 0, a * 16, fr, fq);
          const v8s al = bil_frag_t(s_lo[buf], kBilPitch64, 0, a * 16, fr, fq);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bfr[j], acc[a][j], 0, 0, 0);
            acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bfr[j], acc[a][j], 0, 0, 0);
          }
        }
      }
    }
    if (more) {
      store(buf ^ 1);
      __syncthreads();
    }
  }

  if (p.gb && blockIdx.x == 0 && blockIdx.y == 0) {   // the bias gradient: 32 row sums, added in a fixed order
    if ((tid & 7) == 0) s_gb[tid >> 3] = gsum;
    __syncthreads();
    if (tid == 0) {
      float v = 0.f;
      for (int r = 0; r < kBilRows; ++r) v += s_gb[r];
      p.gb[k] = p.scale * v;
    }
  }

  // accumulator element e of lane (fr, fq): row i0 + 16a + 4fq + e of I, column j0 + jw + 16j + fr of J
  if (!live) return;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int jj = j0 + jw + j * 16 + fr;
      if (jj >= J) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + a * 16 + fq * 4 + e;
        if (i < I) p.gw[((long long)k * I + i) * J + jj] = p.scale * acc[a][j][e];
      }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline bool bil_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// sizes the kernels take: 16-byte rows; k, I / 16 and the tiles of I and J are grid.y / grid.z
static bool bil_sizes(int B, int I, int J, int K) {
  return B > 0 && I > 0 && J > 0 && K > 0 && I % 8 == 0 && J % 8 == 0 && K <= 65535 && I <= 65535 * 16 && J <= 65535 * 64;
}

// y [B][K] bf16 = x1 [B][I] · W [K][I][J] · x2 [B][J] (+ fp32 bias [K] or null)
BIGDL_EXPORT int bigdl_bilinear_forward(const void* x1, const void* x2, const void* w, const float* bias, void* y, int B,
                                        int I, int J, int K, hipStream_t s) {
  if (!bil_sizes(B, I, J, K) || !x1 || !x2 || !w || !y || !bil_al16(x1) || !bil_al16(x2) || !bil_al16(w) ||
      (reinterpret_cast<uintptr_t>(y) & 1) || (reinterpret_cast<uintptr_t>(bias) & 3))
    return (int)hipErrorInvalidValue;
  BilP p{};
  p.x1 = (const bf16_t*)x1; p.x2 = (const bf16_t*)x2; p.w = (const bf16_t*)w; p.bias = bias; p.out = (bf16_t*)y;
  p.B = B; p.I = I; p.J = J; p.K = K;
  const dim3 grid((unsigned)((B + kBilRows - 1) / kBilRows), (unsigned)K);
  hipLaunchKernelGGL(k_bil_u<BIL_FWD>, grid, dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

// which = 1: gx1 [B][I] bf16 from gy [B][K], xo = x2 [B][J];  which = 2: gx2 [B][J] from gy, xo = x1 [B][I]
BIGDL_EXPORT int bigdl_bilinear_gx(int which, const void* gy, const void* xo, const void* w, void* gx, int B, int I, int J,
                                   int K, hipStream_t s) {
  if ((which != 1 && which != 2) || !bil_sizes(B, I, J, K) || !gy || !xo || !w || !gx || !bil_al16(xo) || !bil_al16(w) ||
      !bil_al16(gx) || (reinterpret_cast<uintptr_t>(gy) & 1))
    return (int)hipErrorInvalidValue;
  BilP p{};
  p.gy = (const bf16_t*)gy; p.w = (const bf16_t*)w; p.out = (bf16_t*)gx;
  p.B = B; p.I = I; p.J = J; p.K = K;
  const unsigned bt = (unsigned)((B + kBilRows - 1) / kBilRows);
  if (which == 1) {
    p.x2 = (const bf16_t*)xo;
    hipLaunchKernelGGL(k_bil_u<BIL_GX1>, dim3(bt, (unsigned)((I + 15) / 16)), dim3(256), 0, s, p);
  } else {
    p.x1 = (const bf16_t*)xo;
    hipLaunchKernelGGL(k_bil_v, dim3(bt, (unsigned)((J + kBilJt - 1) / kBilJt)), dim3(256), 0, s, p);
  }
  return (int)hipGetLastError();
}

// gw [K][I][J] fp32 = scale · the weight gradient, gb [K] fp32 (or null) = scale · Σ_b gy (every element written once)
BIGDL_EXPORT int bigdl_bilinear_wgrad(const void* gy, const void* x1, const void* x2, float* gw, float* gb, float scale,
                                      int B, int I, int J, int K, hipStream_t s) {
  if (!bil_sizes(B, I, J, K) || !gy || !x1 || !x2 || !gw || !bil_al16(x1) || !bil_al16(x2) ||
      (reinterpret_cast<uintptr_t>(gy) & 1) || (reinterpret_cast<uintptr_t>(gw) & 3) || (reinterpret_cast<uintptr_t>(gb) & 3))
    return (int)hipErrorInvalidValue;
  BilW p{};
  p.x1 = (const bf16_t*)x1; p.x2 = (const bf16_t*)x2; p.gy = (const bf16_t*)gy; p.gw = gw; p.gb = gb; p.scale = scale;
  p.B = B; p.I = I; p.J = J; p.K = K;
  const dim3 grid((unsigned)((J + kBilJc - 1) / kBilJc), (unsigned)((I + kBilIc - 1) / kBilIc), (unsigned)K);
  hipLaunchKernelGGL(k_bil_wgrad, grid, dim3(256), 0, s, p);
  return (int)hipGetLastError();
}
