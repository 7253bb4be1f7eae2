// Highway (nn/layers/math_ops.py) on the bf16 MFMA: y = t∘h + (1−t)∘x with t = σ(x·Wtᵀ + bt), h = act(x·Whᵀ + bh),
// and its gradients.  x, gy, y, gx are [B][N] bf16; W [2N][N] bf16 is read where the layer keeps it (rows 0..N−1
// the transform gate Wt, rows N..2N−1 the candidate Wh); bias [2N] fp32 or null; act ∈ {identity, tanh, relu,
// sigmoid}.  No pass writes the [B][2N] pre-activation.
//
//   y[b,j]   = t·h + (1−t)·x[b,j]           t, h from the two accumulator sets of column j            k_hw_fwd
//   DG[b,:]  = [gy·(h−x)·t(1−t) | gy·t·act'(h)]      gx = DG·W + gy∘(1−t)                               k_hw_bwd
//   gW[c,i]  = s · Σ_b DG[b,c]·x[b,i]        gb[c] = s · Σ_b DG[b,c]                                   k_hw_wgrad
//
// Tiles: 32 batch rows (two MFMA row fragments) in every kernel.
// k_hw_fwd.  A block owns 32 batch rows and 64 output columns, 16 per wave.  A wave carries two accumulator sets,
// for weight rows j and N + j; both reduce along W's rows, so the two weight slabs are MFMA A operands exactly as
// they lie, read 16 bytes per lane from global memory to registers, the four k-steps of a 128-column chunk issued
// together one chunk ahead.  The x tile [32][128] goes through a two-stage LDS ring (row pitch 17 sixteen-byte
// units, odd) shared by both sets; with N ≤ 128 it is staged once.  Epilogue on the accumulators in fp32: bias,
// sigmoid, activation, the carry term with x[b,j], one rounding to bf16.  In training the gates G = [t | h]
// [B][2N] bf16 are stored as well; at inference only y.
// k_hw_bwd.  A block owns 32 batch rows and 64 columns of gx, 16 per wave, and reduces over the 2N gate columns
// in chunks of 64.  Each thread forms one 16-byte unit of the DG chunk [32][64] in fp32 from gy, G and x (act'
// from the stored h: 1, 1−h², h>0, h(1−h)), rounds it once to bf16 and stores it to LDS as the B operand; the
// W chunk [64 of 2N][64 of N] is staged beside it as it lies and its A fragments are read transposed
// (ds_read_b64_tr_b16).  Both tiles are double-buffered, the global loads of chunk c+1 issued before the MFMAs of
// chunk c.  gy∘(1−t) is added on the accumulators before the single rounding of gx.  The blocks of the first
// column tile also store DG [B][2N] bf16 (each element by exactly one block); with need_input = 0 only those
// blocks are launched and they skip the GEMM.  Every column tile forms the DG chunks of its batch rows again (the
// gy, G and x loads and the gate arithmetic, ⌈N/64⌉ times in all): cheap beside the GEMM at the sizes Highway is
// used at, but a cost that grows with N.
// k_hw_wgrad.  A block owns 64 rows of gW (gate columns c) and 128 columns of N (32 per wave) and sums ALL batch
// rows in stages of 32: each element is written once, no split, no atomics.  Both operands are batch-strided, so
// both fragments are transposed LDS reads.  The blocks of the first N tile also sum their 64 columns of DG, which
// they load anyway: the bias gradient, in a fixed order.
//
// Tails in B and N are zero-filled on load and masked on store; N must be a multiple of 8.  Every result is the
// same bits on every run.
#include "common.h"

typedef short v8s __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s hw_lds_v4s;

constexpr int kHwRows = 32;               // batch rows of a block: two MFMA row fragments
constexpr int kHwNq = kHwRows / 16;
constexpr int kHwKc = 128;                // k_hw_fwd: columns of the reduction staged at a time; k_hw_wgrad: its N tile
constexpr int kHwPitch = kHwKc / 8 + 1;   // row pitch of a 128-column tile, 16-byte units (odd)
constexpr int kHwJt = 64;                 // k_hw_fwd, k_hw_bwd: output columns of a block
constexpr int kHwCc = 64;                 // k_hw_bwd: gate columns staged at a time; k_hw_wgrad: its tile of them
constexpr int kHwPitch64 = 64 / 8 + 1;    // row pitch of a 64-column tile, 16-byte units

enum { HW_IDENTITY = 0, HW_TANH = 1, HW_RELU = 2, HW_SIGMOID = 3 };

struct HwP {
  const bf16_t* x;       // [B][N]
  const bf16_t* w;       // [2N][N]
  const float* bias;     // [2N] or null (forward)
  const bf16_t* gy;      // [B][N] (backward)
  const bf16_t* g;       // gates [B][2N] (backward)
  bf16_t* out;           // y or gx [B][N]
  bf16_t* gates;         // forward: [B][2N] or null
  bf16_t* dg;            // backward: [B][2N]
  int B, N, need_input;
};

__device__ __forceinline__ bigdl_u32x4 hw_ld16(const bf16_t* p, bool on) {
  return on ? *reinterpret_cast<const bigdl_u32x4*>(p) : bigdl_u32x4{0u, 0u, 0u, 0u};
}

__device__ __forceinline__ float hw_sgm(float v) { return 1.f / (1.f + __expf(-v)); }

template <int ACT>
__device__ __forceinline__ float hw_act(float a) {
  return ACT == HW_TANH ? tanhf(a) : ACT == HW_RELU ? fmaxf(a, 0.f) : ACT == HW_SIGMOID ? hw_sgm(a) : a;
}

// act' from the stored activation h
template <int ACT>
__device__ __forceinline__ float hw_dact(float h) {
  return ACT == HW_TANH ? 1.f - h * h : ACT == HW_RELU ? (h > 0.f ? 1.f : 0.f) : ACT == HW_SIGMOID ? h * (1.f - h) : 1.f;
}

__device__ __forceinline__ void hw_unpack4(uint2 u, float* o) {
  o[0] = __uint_as_float(u.x << 16);
  o[1] = __uint_as_float(u.x & 0xFFFF0000u);
  o[2] = __uint_as_float(u.y << 16);
  o[3] = __uint_as_float(u.y & 0xFFFF0000u);
}

__device__ __forceinline__ uint2 hw_pack4(const float* v) {
  return make_uint2((uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16), (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16));
}

// Transposed fragment of a row-major bf16 LDS tile (pitch in 16-byte units): lane (fr, fq) receives column
// col + fr of rows r0 + 8fq .. r0 + 8fq + 7.  Lane 4q + p of a 16-lane group addresses row r0 + 8fq + q, columns
// col + 4p .. + 3.
__device__ __forceinline__ v8s hw_frag_t(const bigdl_u32x4* tile, int pitch, int r0, int col, int fr, int fq) {
  const bf16_t* base = reinterpret_cast<const bf16_t*>(tile) + (r0 + 8 * fq + (fr >> 2)) * pitch * 8 + col + 4 * (fr & 3);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((hw_lds_v4s*)base);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((hw_lds_v4s*)(base + 4 * pitch * 8));
  return v8s{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ------------------------------------------------------------------------------------------------
// forward: two accumulator sets per output column, the gate epilogue on them
// ------------------------------------------------------------------------------------------------
template <int ACT>
__global__ void __launch_bounds__(256) k_hw_fwd(HwP p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 lds[2][kHwRows * kHwPitch];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * kHwRows, j0 = blockIdx.y * kHwJt + wid * 16;
  const int B = p.B, N = p.N;
  const int nch = (N + kHwKc - 1) / kHwKc;
  const bool ring = nch > 1;   // with one chunk the x tile is staged once and stays in lds[0]
  const bool live = j0 < N;    // a wave whose 16 columns lie beyond N only helps staging
  const int jr = j0 + fr;      // this lane's weight rows: jr (gate) and N + jr (candidate)

  bigdl_u32x4 wt[4], wh[4], nt[4], nh[4];
  auto load_w = [&](int c, bigdl_u32x4(&dt)[4], bigdl_u32x4(&dh)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = c * kHwKc + s * 32 + fq * 8;
      const bool on = jr < N && k < N;
      dt[s] = hw_ld16(p.w + (long long)jr * N + k, on);
      dh[s] = hw_ld16(p.w + ((long long)N + jr) * N + k, on);
    }
  };
  // the x tile of chunk c: one 16-byte unit per thread and pass, rows ≥ B and columns ≥ N zero
  bigdl_u32x4 xs[kHwRows * (kHwKc / 8) / 256];
  auto load_x = [&](int c) {
#pragma unroll
    for (int r = 0; r < kHwRows * (kHwKc / 8) / 256; ++r) {
      const int idx = r * 256 + tid, k = c * kHwKc + (idx & 15) * 8, n = n0 + (idx >> 4);
      xs[r] = hw_ld16(p.x + (long long)n * N + k, n < B && k < N);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int r = 0; r < kHwRows * (kHwKc / 8) / 256; ++r) {
      const int idx = r * 256 + tid;
      lds[buf][(idx >> 4) * kHwPitch + (idx & 15)] = xs[r];
    }
  };

  v4f at[kHwNq], ah[kHwNq];
#pragma unroll
  for (int q = 0; q < kHwNq; ++q) at[q] = ah[q] = v4f{0.f, 0.f, 0.f, 0.f};

  load_w(0, wt, wh);
  load_x(0);
  store_x(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int buf = ring ? (c & 1) : 0;
    const bool more = c + 1 < nch;
    if (more) {
      load_w(c + 1, nt, nh);
      load_x(c + 1);
    }
    if (live) {
      const int nks = (min(kHwKc, N - c * kHwKc) + 31) >> 5;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < nks) {
#pragma unroll
          for (int q = 0; q < kHwNq; ++q) {
            const v8s xf = __builtin_bit_cast(v8s, lds[buf][(q * 16 + fr) * kHwPitch + s * 4 + fq]);
            at[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8s, wt[s]), xf, at[q], 0, 0, 0);
            ah[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8s, wh[s]), xf, ah[q], 0, 0, 0);
          }
        }
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        wt[s] = nt[s];
        wh[s] = nh[s];
      }
      store_x(buf ^ 1);
      __syncthreads();
    }
  }

  // accumulator element e of lane (fr, fq) of fragment q: row n0 + 16q + fr, column j0 + 4fq + e
  const int j = j0 + fq * 4;
  if (!live || j >= N) return;
  float bt[4], bh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bt[e] = p.bias ? p.bias[j + e] : 0.f;
    bh[e] = p.bias ? p.bias[N + j + e] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < kHwNq; ++q) {
    const int n = n0 + q * 16 + fr;
    if (n >= B) continue;
    float xe[4], t[4], h[4], y[4];
    hw_unpack4(*reinterpret_cast<const uint2*>(p.x + (long long)n * N + j), xe);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t[e] = hw_sgm(at[q][e] + bt[e]);
      h[e] = hw_act<ACT>(ah[q][e] + bh[e]);
      y[e] = t[e] * h[e] + (1.f - t[e]) * xe[e];
    }
    *reinterpret_cast<uint2*>(p.out + (long long)n * N + j) = hw_pack4(y);
    if (p.gates) {
      *reinterpret_cast<uint2*>(p.gates + (long long)n * 2 * N + j) = hw_pack4(t);
      *reinterpret_cast<uint2*>(p.gates + (long long)n * 2 * N + N + j) = hw_pack4(h);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward: DG formed chunk by chunk on the way into gx = DG·W + gy∘(1−t)
// ------------------------------------------------------------------------------------------------
template <int ACT>
__global__ void __launch_bounds__(256) k_hw_bwd(HwP p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_w[2][kHwCc * kHwPitch64];     // [64 of 2N][64 of N]
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_d[2][kHwRows * kHwPitch64];   // [32 rows][64 of 2N]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * kHwRows, i0 = blockIdx.y * kHwJt;
  const int B = p.B, N = p.N, C2 = 2 * N;
  const int nch = (C2 + kHwCc - 1) / kHwCc;
  const bool gemm = p.need_input != 0, first = blockIdx.y == 0;
  const int n = n0 + (tid >> 3);   // this thread's row of the DG chunk; its unit is columns 8·(tid & 7) .. + 7

  // a chunk's operands: W[c0 .. +63][i0 .. +63] (two units per thread) and this thread's unit of gy, t, h, x
  bigdl_u32x4 ws[2], gyv, tv, hv, xv;
  auto load = [&](int c) {
    if (gemm) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int idx = r * 256 + tid, cr = c * kHwCc + (idx >> 3), i = i0 + (idx & 7) * 8;
        ws[r] = hw_ld16(p.w + (long long)cr * N + i, cr < C2 && i < N);
      }
    }
    const int cc = c * kHwCc + (tid & 7) * 8, cj = cc < N ? cc : cc - N;   // N % 8 == 0: a unit lies in one half
    const bool on = n < B && cc < C2;
    gyv = hw_ld16(p.gy + (long long)n * N + cj, on);
    tv = hw_ld16(p.g + (long long)n * C2 + cj, on);
    hv = hw_ld16(p.g + (long long)n * C2 + N + cj, on);
    xv = hw_ld16(p.x + (long long)n * N + cj, on && cc < N);
  };
  // DG's unit in fp32, rounded once; to LDS (buf ≥ 0) and, from the first column tile, to global memory
  auto emit = [&](int c, int buf) {
    const int cc = c * kHwCc + (tid & 7) * 8;
    const bool gate = cc < N;
    bigdl_u32x4 dv;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      uint32_t wv = 0;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        auto el = [&](uint32_t v) { return e ? __uint_as_float(v & 0xFFFF0000u) : __uint_as_float(v << 16); };
        const float gv = el(gyv[u]), t = el(tv[u]), h = el(hv[u]), x = el(xv[u]);
        const float dgv = gate ? gv * (h - x) * (t * (1.f - t)) : gv * t * hw_dact<ACT>(h);
        wv |= (uint32_t)f2bf(dgv) << (16 * e);
      }
      dv[u] = wv;
    }
    if (buf >= 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int idx = r * 256 + tid;
        s_w[buf][(idx >> 3) * kHwPitch64 + (idx & 7)] = ws[r];
      }
      s_d[buf][(tid >> 3) * kHwPitch64 + (tid & 7)] = dv;
    }
    if (first && n < B && cc < C2) *reinterpret_cast<bigdl_u32x4*>(p.dg + (long long)n * C2 + cc) = dv;
  };

  if (!gemm) {   // no input gradient wanted: DG only
    for (int c = 0; c < nch; ++c) {
      load(c);
      emit(c, -1);
    }
    return;
  }

  v4f acc[kHwNq];
#pragma unroll
  for (int q = 0; q < kHwNq; ++q) acc[q] = v4f{0.f, 0.f, 0.f, 0.f};

  const bool live = i0 + wid * 16 < N;   // a wave whose 16 columns lie beyond N only helps staging
  load(0);
  emit(0, 0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nch;
    if (more) load(c + 1);
    if (live) {
      const int nks = (min(kHwCc, C2 - c * kHwCc) + 31) >> 5;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s < nks) {
          const v8s af = hw_frag_t(s_w[buf], kHwPitch64, s * 32, wid * 16, fr, fq);
#pragma unroll
          for (int q = 0; q < kHwNq; ++q) {
            const v8s df = __builtin_bit_cast(v8s, s_d[buf][(q * 16 + fr) * kHwPitch64 + s * 4 + fq]);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, df, acc[q], 0, 0, 0);
          }
        }
      }
    }
    if (more) {
      emit(c + 1, buf ^ 1);
      __syncthreads();
    }
  }

  // accumulator element e of lane (fr, fq) of fragment q: row n0 + 16q + fr, column i0 + 16·wave + 4fq + e
  const int i = i0 + wid * 16 + fq * 4;
  if (!live || i >= N) return;
#pragma unroll
  for (int q = 0; q < kHwNq; ++q) {
    const int m = n0 + q * 16 + fr;
    if (m >= B) continue;
    float gv[4], t[4], o[4];
    hw_unpack4(*reinterpret_cast<const uint2*>(p.gy + (long long)m * N + i), gv);
    hw_unpack4(*reinterpret_cast<const uint2*>(p.g + (long long)m * C2 + i), t);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = acc[q][e] + gv[e] * (1.f - t[e]);
    *reinterpret_cast<uint2*>(p.out + (long long)m * N + i) = hw_pack4(o);
  }
}

// ------------------------------------------------------------------------------------------------
// gW[c][i] = scale · Σ_b DG[b][c] · x[b][i],  gb[c] = scale · Σ_b DG[b][c]
// ------------------------------------------------------------------------------------------------
struct HwW {
  const bf16_t* dg;   // [B][2N]
  const bf16_t* x;    // [B][N]
  float* gw;          // [2N][N]
  float* gb;          // [2N] or null: summed by the blocks of the first N tile
  float scale;
  int B, N;
};

__global__ void __launch_bounds__(256) k_hw_wgrad(HwW p) {
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_d[2][kHwRows * kHwPitch64];   // [32 rows][64 of 2N]
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 s_x[2][kHwRows * kHwPitch];     // [32 rows][128 of N]
  __shared__ float s_gb[kHwRows][kHwCc];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int i0 = blockIdx.x * kHwKc, c0 = blockIdx.y * kHwCc;
  const int B = p.B, N = p.N, C2 = 2 * N;
  const bool bias = p.gb != nullptr && blockIdx.x == 0;

  bigdl_u32x4 dv, xv[2];
  float gsum[8];   // this thread's unit of DG's stage row, summed over all stages
#pragma unroll
  for (int e = 0; e < 8; ++e) gsum[e] = 0.f;
  auto load = [&](int b0) {
    const int n = b0 + (tid >> 3), c = c0 + (tid & 7) * 8;
    dv = hw_ld16(p.dg + (long long)n * C2 + c, n < B && c < C2);
    if (bias) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        gsum[2 * u] += __uint_as_float(dv[u] << 16);
        gsum[2 * u + 1] += __uint_as_float(dv[u] & 0xFFFF0000u);
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int idx = r * 256 + tid, m = b0 + (idx >> 4), i = i0 + (idx & 15) * 8;
      xv[r] = hw_ld16(p.x + (long long)m * N + i, m < B && i < N);
    }
  };
  auto store = [&](int buf) {
    s_d[buf][(tid >> 3) * kHwPitch64 + (tid & 7)] = dv;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int idx = r * 256 + tid;
      s_x[buf][(idx >> 4) * kHwPitch + (idx & 15)] = xv[r];
    }
  };

  v4f acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[a][j] = v4f{0.f, 0.f, 0.f, 0.f};

  const int nst = (B + kHwRows - 1) / kHwRows;
  const int iw = wid * 32;   // this wave's 32 columns of the N tile
  const bool live = i0 + iw < N;
  load(0);
  store(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nst;
    if (more) load((st + 1) * kHwRows);
    if (live) {
      v8s bfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = hw_frag_t(s_x[buf], kHwPitch, 0, iw + j * 16, fr, fq);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (c0 + a * 16 < C2) {
          const v8s ad = hw_frag_t(s_d[buf], kHwPitch64, 0, a * 16, fr, fq);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, bfr[j], acc[a][j], 0, 0, 0);
        }
      }
    }
    if (more) {
      store(buf ^ 1);
      __syncthreads();
    }
  }

  if (bias) {   // the bias gradient: 32 row sums per column, added in a fixed order
#pragma unroll
    for (int e = 0; e < 8; ++e) s_gb[tid >> 3][(tid & 7) * 8 + e] = gsum[e];
    __syncthreads();
    if (tid < kHwCc && c0 + tid < C2) {
      float v = 0.f;
      for (int r = 0; r < kHwRows; ++r) v += s_gb[r][tid];
      p.gb[c0 + tid] = p.scale * v;
    }
  }

  // accumulator element e of lane (fr, fq): row c0 + 16a + 4fq + e of gW, column i0 + iw + 16j + fr
  if (!live) return;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = i0 + iw + j * 16 + fr;
      if (i >= N) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + a * 16 + fq * 4 + e;
        if (c < C2) p.gw[(long long)c * N + i] = p.scale * acc[a][j][e];
      }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline bool hw_al(const void* q, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) == 0; }

// sizes the kernels take: 16-byte rows; the column tiles are grid.y
static bool hw_sizes(int B, int N) { return B > 0 && N > 0 && N % 8 == 0 && N <= 65535 * (kHwCc / 2); }

template <template <int> class L>
static void hw_launch_act(int act, dim3 grid, hipStream_t s, const HwP& p) {
  switch (act) {
    case HW_TANH: L<HW_TANH>::go(grid, s, p); break;
    case HW_RELU: L<HW_RELU>::go(grid, s, p); break;
    case HW_SIGMOID: L<HW_SIGMOID>::go(grid, s, p); break;
    default: L<HW_IDENTITY>::go(grid, s, p); break;
  }
}
template <int ACT> struct HwFwd {
  static void go(dim3 grid, hipStream_t s, const HwP& p) { hipLaunchKernelGGL(k_hw_fwd<ACT>, grid, dim3(256), 0, s, p); }
};
template <int ACT> struct HwBwd {
  static void go(dim3 grid, hipStream_t s, const HwP& p) { hipLaunchKernelGGL(k_hw_bwd<ACT>, grid, dim3(256), 0, s, p); }
};

// y [B][N] bf16 = t∘h + (1−t)∘x from x [B][N], W [2N][N] (+ fp32 bias [2N] or null); gates [B][2N] bf16 or null
BIGDL_EXPORT int bigdl_highway_forward(const void* x, const void* w, const float* bias, void* y, void* gates, int B, int N,
                                       int act, hipStream_t s) {
  if (!hw_sizes(B, N) || act < 0 || act > 3 || !x || !w || !y || !hw_al(x, 15) || !hw_al(w, 15) || !hw_al(y, 15) ||
      !hw_al(gates, 15) || !hw_al(bias, 3))
    return (int)hipErrorInvalidValue;
  HwP p{};
  p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.bias = bias; p.out = (bf16_t*)y; p.gates = (bf16_t*)gates;
  p.B = B; p.N = N;
  hw_launch_act<HwFwd>(act, dim3((unsigned)((B + kHwRows - 1) / kHwRows), (unsigned)((N + kHwJt - 1) / kHwJt)), s, p);
  BIGDL_CHECK_LAUNCH();
}

// dg [B][2N] bf16 = the gate gradients from gy, gates, x; with need_input also gx [B][N] bf16 = dg·W + gy∘(1−t)
BIGDL_EXPORT int bigdl_highway_backward(const void* gy, const void* x, const void* gates, const void* w, void* gx, void* dg,
                                        int B, int N, int act, int need_input, hipStream_t s) {
  if (!hw_sizes(B, N) || act < 0 || act > 3 || !gy || !x || !gates || !dg || !hw_al(gy, 15) || !hw_al(x, 15) ||
      !hw_al(gates, 15) || !hw_al(dg, 15) || (need_input && (!w || !gx || !hw_al(w, 15) || !hw_al(gx, 15))))
    return (int)hipErrorInvalidValue;
  HwP p{};
  p.gy = (const bf16_t*)gy; p.x = (const bf16_t*)x; p.g = (const bf16_t*)gates; p.w = (const bf16_t*)w;
  p.out = (bf16_t*)gx; p.dg = (bf16_t*)dg;
  p.B = B; p.N = N; p.need_input = need_input ? 1 : 0;
  const unsigned ct = need_input ? (unsigned)((N + kHwJt - 1) / kHwJt) : 1u;
  hw_launch_act<HwBwd>(act, dim3((unsigned)((B + kHwRows - 1) / kHwRows), ct), s, p);
  BIGDL_CHECK_LAUNCH();
}

// gw [2N][N] fp32 = scale · dgᵀ·x, gb [2N] fp32 (or null) = scale · Σ_b dg (every element written once)
BIGDL_EXPORT int bigdl_highway_wgrad(const void* dg, const void* x, float* gw, float* gb, float scale, int B, int N,
                                     hipStream_t s) {
  if (!hw_sizes(B, N) || !dg || !x || !gw || !hw_al(dg, 15) || !hw_al(x, 15) || !hw_al(gw, 3) || !hw_al(gb, 3))
    return (int)hipErrorInvalidValue;
  HwW p{};
  p.dg = (const bf16_t*)dg; p.x = (const bf16_t*)x; p.gw = gw; p.gb = gb; p.scale = scale;
  p.B = B; p.N = N;
  const dim3 grid((unsigned)((N + kHwKc - 1) / kHwKc), (unsigned)((2 * N + kHwCc - 1) / kHwCc));
  hipLaunchKernelGGL(k_hw_wgrad, grid, dim3(256), 0, s, p);
  BIGDL_CHECK_LAUNCH();
}
