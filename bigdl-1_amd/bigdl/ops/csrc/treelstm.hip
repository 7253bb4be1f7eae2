// BinaryTreeLSTM (nn/layers/tree_lstm.py) on the bf16 MFMA: one fused gather-GEMM-gate launch per tree level,
// forward and backward.  All trees of a batch are grouped by node height on the host (the plan, one int32
// upload); level 0 is the dense leaf row space [B·L], levels 1.. hold the composer nodes.
//
//   leaf      c = Wc·x + bc                 h = σ(Wo·x + bo) ⊙ tanh c     (h = tanh c without the output gate)
//   composer  i, lf, rf, o = σ(L·lh + R·rh + b)   u = tanh(L·lh + R·rh + b)
//             c = i⊙u + lf⊙lc + rf⊙rc        h = o ⊙ tanh c
//
// Tiling.  A block of 4 waves owns 32 level rows × 16 hidden units and ALL gate tiles of those units
// (5 / 4 composer, 2 / 1 leaf, 1 backward), so the cell update runs on the MFMA accumulators with no
// exchange between gates.  The A operand is gathered: the rows' [lh | rh] (K = 2H), their embedding row
// (K = inputSize) or, backward, their parent's gate-gradient row (K = G·H8), fetched by plan index once
// per block into LDS in stages of 512 columns.  Each K half is zero-filled to a multiple of 32, so any
// even size works; the LDS row pitch is 65 sixteen-byte units (odd), which keeps the 16 row lanes of a
// fragment read on distinct banks.  The waves split K in 32-column chunks (wave w takes chunks w, w+4, ..),
// read the packed weights straight from global memory (a weight fragment is used by one wave of one
// block; reuse across row tiles is L2's) and fold their partial tiles through LDS into wave 0, which has
// prefetched lc / rc by child index and writes c (fp32) and h (bf16) at the node's row plus, in training,
// the activations, tanh c and the gathered operand rows in level-row order for the backward and the
// weight-gradient GEMMs.  Pad rows (node −1) write nothing.
//
// Backward is the same body in gather form: dh = gy[node] + DG[parent] · W_sideᵀ.  The plan orders a
// level so that left and right children fill whole 32-row tiles; a tile then multiplies by one weight
// block.  The kernel does not rely on it: it masks rows by side and skips a side no row of the tile has,
// which is how the dense leaf row space (mixed sides) is served by the same code.  Every node has one
// parent, so there are no atomics and the result is the same bits on every run.
#include "common.h"

typedef short v8s __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

#if defined(__HIP_DEVICE_COMPILE__)
#define BIGDL_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define BIGDL_NO_PK_F32
#endif

constexpr int kTlRows = 32;     // level rows per block
constexpr int kTlStage = 512;   // K columns staged in LDS at a time
constexpr int kTlPitch = kTlStage / 8 + 1;   // LDS row pitch, 16-byte units

__host__ __device__ inline int tl_up(int n, int m) { return (n + m - 1) / m * m; }

struct TlP {
  const int *node, *lk, *rk, *prow, *side;   // this level's plan rows (prow / side: backward)
  int rows;                                  // multiple of 32
  int H, Hp, in;                             // Hp = H rounded up to 8
  const bf16_t* a;      // gather source: h [nodes][H] / x [B·L][in] / composer DG [rows][G·Hp]
  const bf16_t* w;      // packed weights [tiles][Hp16][K] (backward: [side][Hp16][K])
  const float* bias;    // forward: [tiles][Hp16]
  float* c;             // [nodes][H]
  bf16_t* h;            // [nodes][H]
  float* act;           // level-row saves: composer [rows][G][H]; leaf [rows][H] (o)
  float* tc;            // [rows][H]
  bf16_t* xs;           // gathered operand rows [rows][segments · seglen rounded up to 8]
  const bf16_t* gy;     // backward: output gradient [nodes][H]
  const float* pact;    // composer activations, all levels (parent rows)
  const float* pdc;     // composer dc, all levels (parent rows)
  bf16_t* dg;           // backward out: gate gradients [rows][G·Hp]
  float* dc;            // backward out (composer): [rows][H]
};

__device__ __forceinline__ float tl_sgm(float x) { return 1.f / (1.f + __expf(-x)); }

// MODE 0 composer forward, 1 leaf forward, 2 composer backward, 3 leaf backward; GO = output gate
template <int MODE, bool GO>
__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_treelstm(TlP p) {
  constexpr int GC = GO ? 5 : 4;   // composer gates
  constexpr int GL = GO ? 2 : 1;   // leaf gates
  constexpr int NT = MODE == 0 ? GC : MODE == 1 ? GL : 1;   // accumulator tiles per 16 rows
  constexpr bool BWD = MODE >= 2;
  __shared__ __attribute__((aligned(16))) bigdl_u32x4 lds[kTlRows * kTlPitch];
  __shared__ int s_src[2][kTlRows];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int H = p.H, Hp = p.Hp, Hp16 = tl_up(H, 16);
  const int row0 = blockIdx.x * kTlRows, ub = blockIdx.y * 16;
  const int nseg = MODE == 0 ? 2 : 1;
  const int seglen = MODE == 0 ? H : MODE == 1 ? p.in : GC * Hp;
  const int segpitch = tl_up(seglen, 32), K = nseg * segpitch;
  const int segsave = tl_up(seglen, 8);

  v4f acc[2][NT];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int g = 0; g < NT; ++g) acc[q][g] = v4f{0.f, 0.f, 0.f, 0.f};

  // composer forward: the children's c, in flight under the reduction (wave 0 runs the epilogue)
  float pre[2][2][4];
  if constexpr (MODE == 0) {
    if (wid == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int r = row0 + q * 16 + fr;
        const bool v = p.node[r] >= 0;
        const long long lo = v ? (long long)p.lk[r] * H : 0, ro = v ? (long long)p.rk[r] * H : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int u = ub + fq * 4 + e;
          pre[q][0][e] = (v && u < H) ? p.c[lo + u] : 0.f;
          pre[q][1][e] = (v && u < H) ? p.c[ro + u] : 0.f;
        }
      }
    }
  }

  uint32_t* lds32 = reinterpret_cast<uint32_t*>(lds);
  for (int pass = 0; pass < (BWD ? 2 : 1); ++pass) {
    // source row of every tile row (−1: zeros)
    int have = 0;
    if (tid < kTlRows) {
      const int r = row0 + tid, nd = p.node[r];
      int s0 = -1, s1 = -1;
      if (nd >= 0) {
        if constexpr (MODE == 0) { s0 = p.lk[r]; s1 = p.rk[r]; }
        else if constexpr (MODE == 1) s0 = r;
        else s0 = p.side[r] == pass ? p.prow[r] : -1;
      }
      s_src[0][tid] = s0;
      s_src[1][tid] = s1;
      have = s0 >= 0;
    }
    if (!__syncthreads_or(have)) continue;   // block-uniform: no row of this tile needs this pass

    const bf16_t* wbase = p.w + (BWD ? (long long)pass * Hp16 * K : 0);
    for (int k0 = 0; k0 < K; k0 += kTlStage) {
      const int ws = min(kTlStage, K - k0), ws2 = ws >> 1;
      for (int idx = tid; idx < kTlRows * ws2; idx += 256) {
        const int row = idx / ws2, pr = idx - row * ws2, k = k0 + 2 * pr;
        const int seg = (MODE == 0 && k >= segpitch) ? 1 : 0, col = k - seg * segpitch;
        const int src = s_src[seg][row];
        uint32_t v = 0u;
        if (src >= 0 && col < seglen) {
          v = *reinterpret_cast<const uint32_t*>(p.a + (long long)src * seglen + col);
          if (!BWD && p.xs && blockIdx.y == 0)
            *reinterpret_cast<uint32_t*>(p.xs + (long long)(row0 + row) * nseg * segsave + seg * segsave + col) = v;
        }
        lds32[row * (kTlPitch * 4) + pr] = v;
      }
      __syncthreads();
      const int nch = ws >> 5;
      for (int kc = wid; kc < nch; kc += 4) {
        v8s xf[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) xf[q] = __builtin_bit_cast(v8s, lds[(q * 16 + fr) * kTlPitch + kc * 4 + fq]);
        const bf16_t* wp = wbase + (long long)(ub + fr) * K + k0 + kc * 32 + fq * 8;
        bigdl_u32x4 wv[NT];
#pragma unroll
        for (int g = 0; g < NT; ++g) wv[g] = *reinterpret_cast<const bigdl_u32x4*>(wp + (long long)g * Hp16 * K);
#pragma unroll
        for (int g = 0; g < NT; ++g)
#pragma unroll
          for (int q = 0; q < 2; ++q)
            acc[q][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8s, wv[g]), xf[q], acc[q][g], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  // fold the K split into wave 0 through LDS (the staging area is free: every pass ended on a barrier)
  __syncthreads();
  if (wid > 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int g = 0; g < NT; ++g)
        lds[((wid - 1) * 2 * NT + q * NT + g) * 64 + lane] = __builtin_bit_cast(bigdl_u32x4, acc[q][g]);
  }
  __syncthreads();
  if (wid > 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int g = 0; g < NT; ++g) acc[q][g] += __builtin_bit_cast(v4f, lds[(w * 2 * NT + q * NT + g) * 64 + lane]);

#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = row0 + q * 16 + fr;
    const int nd = p.node[r];
    if (nd < 0) continue;
    const long long no = (long long)nd * H, so = (long long)r * H;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int u = ub + fq * 4 + e;
      if (u >= H) continue;
      if constexpr (MODE == 0) {
        float v[GC];
#pragma unroll
        for (int g = 0; g < GC; ++g) v[g] = acc[q][g][e] + p.bias[g * Hp16 + u];
        const float i = tl_sgm(v[0]), lf = tl_sgm(v[1]), rf = tl_sgm(v[2]), uu = tanhf(v[3]);
        const float cc = i * uu + lf * pre[q][0][e] + rf * pre[q][1][e];
        const float t = tanhf(cc);
        float o = 1.f;
        if constexpr (GO) o = tl_sgm(v[4]);
        p.c[no + u] = cc;
        p.h[no + u] = f2bf(o * t);
        if (p.act) {
          float* a = p.act + so * GC + u;
          a[0] = i; a[H] = lf; a[2 * H] = rf; a[3 * H] = uu;
          if constexpr (GO) a[4 * H] = o;
          p.tc[so + u] = t;
        }
      } else if constexpr (MODE == 1) {
        const float cc = acc[q][0][e] + p.bias[u];
        const float t = tanhf(cc);
        float o = 1.f;
        if constexpr (GO) o = tl_sgm(acc[q][1][e] + p.bias[Hp16 + u]);
        p.c[no + u] = cc;
        p.h[no + u] = f2bf(o * t);
        if (p.tc) {
          if constexpr (GO) p.act[so + u] = o;
          p.tc[so + u] = t;
        }
      } else {
        const float dh = bf2f(p.gy[no + u]) + acc[q][0][e];
        const int pr = p.prow[r];
        float dcp = 0.f;
        if (pr >= 0) dcp = p.pdc[(long long)pr * H + u] * p.pact[((long long)pr * GC + 1 + p.side[r]) * H + u];
        const float t = p.tc[so + u];
        if constexpr (MODE == 2) {
          const float* a = p.act + so * GC + u;
          const float i = a[0], lf = a[H], rf = a[2 * H], uu = a[3 * H];
          float o = 1.f;
          if constexpr (GO) o = a[4 * H];
          const float dc = dcp + dh * o * (1.f - t * t);
          const float lc = p.c[(long long)p.lk[r] * H + u], rc = p.c[(long long)p.rk[r] * H + u];
          bf16_t* d = p.dg + (long long)r * GC * Hp + u;
          d[0] = f2bf(dc * uu * i * (1.f - i));
          d[Hp] = f2bf(dc * lc * lf * (1.f - lf));
          d[2 * Hp] = f2bf(dc * rc * rf * (1.f - rf));
          d[3 * Hp] = f2bf(dc * i * (1.f - uu * uu));
          if constexpr (GO) d[4 * Hp] = f2bf(dh * t * o * (1.f - o));
          p.dc[so + u] = dc;
        } else {
          float o = 1.f;
          if constexpr (GO) o = p.act[so + u];
          bf16_t* d = p.dg + (long long)r * GL * Hp + u;
          d[0] = f2bf(dcp + dh * o * (1.f - t * t));
          if constexpr (GO) d[Hp] = f2bf(dh * t * o * (1.f - o));
        }
      }
    }
  }
}

// LDS bytes of a level kernel (the 512-column staging area, which also holds the fold), or −1 for sizes the
// kernels do not take: odd H or inputSize (operand rows are gathered in bf16 pairs).
BIGDL_EXPORT long long bigdl_treelstm_lds_bytes(int H, int in, int G) {
  if (H <= 0 || in <= 0 || H % 2 || in % 2 || (G != 4 && G != 5)) return -1;
  return (long long)kTlRows * kTlPitch * 16 + 2 * kTlRows * 4;
}

static int tl_launch(int mode, int go, const TlP& p, hipStream_t s) {
  if (p.rows <= 0 || p.rows % kTlRows || bigdl_treelstm_lds_bytes(p.H, p.in, go ? 5 : 4) < 0 || !p.node || !p.a || !p.w)
    return (int)hipErrorInvalidValue;
  if (mode == 0 ? !(p.lk && p.rk && p.bias && p.c && p.h) : mode == 1 ? !(p.bias && p.c && p.h)
      : !(p.prow && p.side && p.gy && p.tc && p.dg && (mode == 3 || (p.lk && p.rk && p.c && p.act && p.dc))))
    return (int)hipErrorInvalidValue;
  if (mode <= 1 && (p.act || p.tc || p.xs) && !(p.tc && p.xs && (p.act || (mode == 1 && !go)))) return (int)hipErrorInvalidValue;
  if (mode == 3 && go && !p.act) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(p.rows / kTlRows), (unsigned)(tl_up(p.H, 16) / 16)), blk(256);
#define TL_GO(M)                                                         \
  if (go) hipLaunchKernelGGL((k_treelstm<M, true>), grid, blk, 0, s, p); \
  else hipLaunchKernelGGL((k_treelstm<M, false>), grid, blk, 0, s, p)
  switch (mode) {
    case 0: TL_GO(0); break;
    case 1: TL_GO(1); break;
    case 2: TL_GO(2); break;
    case 3: TL_GO(3); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef TL_GO
  return (int)hipGetLastError();
}

// One level.  plan = int32 [5][R] (node, left, right, parent row, side); the level is plan rows
// [row0, row0 + rows); save buffers (act, tc, xs, dg, dc) point at the level's first row.
BIGDL_EXPORT int bigdl_treelstm_level(int mode, int go, const int* plan, long long R, long long row0, int rows, int H,
                                      int in, const void* a, const void* w, const float* bias, float* c, void* h,
                                      float* act, float* tc, void* xs, const void* gy, const float* pact,
                                      const float* pdc, void* dg, float* dc, hipStream_t s) {
  if (!plan || row0 < 0 || rows <= 0 || row0 + rows > R) return (int)hipErrorInvalidValue;
  TlP p{};
  p.node = plan + row0; p.lk = plan + R + row0; p.rk = plan + 2 * R + row0;
  p.prow = plan + 3 * R + row0; p.side = plan + 4 * R + row0;
  p.rows = rows; p.H = H; p.Hp = tl_up(H, 8); p.in = in;
  p.a = (const bf16_t*)a; p.w = (const bf16_t*)w; p.bias = bias; p.c = c; p.h = (bf16_t*)h;
  p.act = act; p.tc = tc; p.xs = (bf16_t*)xs; p.gy = (const bf16_t*)gy; p.pact = pact; p.pdc = pdc;
  p.dg = (bf16_t*)dg; p.dc = dc;
  return tl_launch(mode, go, p, s);
}

// Whole tree, forward.  lvl[0] = leaf rows R0, lvl[1..nlev-1] = composer rows per height (host array, each a
// multiple of 32); composer saves are indexed by plan row − R0.  Saves null = inference.
BIGDL_EXPORT int bigdl_treelstm_fwd(int go, const int* plan, long long R, const int* lvl, int nlev, int H, int in,
                                    const void* x, const void* wl, const float* bl, const void* wc, const float* bc,
                                    float* c, void* h, float* act_l, float* tc_l, void* xs_l, float* act_c,
                                    float* tc_c, void* xs_c, hipStream_t s) {
  if (nlev < 1 || !lvl) return (int)hipErrorInvalidValue;
  const int G = go ? 5 : 4, Hp = tl_up(H, 8);
  int rc = bigdl_treelstm_level(1, go, plan, R, 0, lvl[0], H, in, x, wl, bl, c, h, act_l, tc_l, xs_l, nullptr, nullptr,
                                nullptr, nullptr, nullptr, s);
  long long r = 0;   // composer-space row
  for (int l = 1; l < nlev && !rc; ++l) {
    if (lvl[l] > 0)
      rc = bigdl_treelstm_level(0, go, plan, R, lvl[0] + r, lvl[l], H, in, h, wc, bc, c, h,
                                act_c ? act_c + r * G * H : nullptr, tc_c ? tc_c + r * H : nullptr,
                                xs_c ? (bf16_t*)xs_c + r * 2 * Hp : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s);
    r += lvl[l];
  }
  return rc;
}

// Whole tree, backward: root level down to the leaves.  wt = the transposed packs [2][Hp16][K].
BIGDL_EXPORT int bigdl_treelstm_bwd(int go, const int* plan, long long R, const int* lvl, int nlev, int H, int in,
                                    const void* gy, const void* wt, float* c, float* act_l, float* tc_l, float* act_c,
                                    float* tc_c, void* dg_l, void* dg_c, float* dc_c, hipStream_t s) {
  if (nlev < 1 || !lvl) return (int)hipErrorInvalidValue;
  const int G = go ? 5 : 4, Hp = tl_up(H, 8);
  long long r = 0;
  for (int l = 1; l < nlev; ++l) r += lvl[l];
  // a tree of leaves only has no composer rows: the gather source is never read, any non-null pointer serves
  const void* a = dg_c ? dg_c : gy;
  int rc = 0;
  for (int l = nlev - 1; l >= 1 && !rc; --l) {
    r -= lvl[l];
    if (lvl[l] > 0)
      rc = bigdl_treelstm_level(2, go, plan, R, lvl[0] + r, lvl[l], H, in, a, wt, nullptr, c, nullptr,
                                act_c + r * G * H, tc_c + r * H, nullptr, gy, act_c, dc_c, (bf16_t*)dg_c + r * G * Hp,
                                dc_c + r * H, s);
  }
  if (!rc)
    rc = bigdl_treelstm_level(3, go, plan, R, 0, lvl[0], H, in, a, wt, nullptr, c, nullptr, act_l, tc_l, nullptr, gy,
                              act_c, dc_c, dg_l, nullptr, s);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// Weight packs (once per call) from the bf16 parameters w0 / w1 and the fp32 biases b0 / b1:
//   mode 0  composer forward  dst[g][j16][Wl row | Wr row, each half padded to 32]   bias = bl + br
//   mode 1  leaf forward      dst[g][j16][in padded to 32], g = (c, o)               bias = (bc, bo)
//   mode 2  composer backward dst[side][k16][g·Hp + j] = W_side[g·H + j][k]
//   mode 3  leaf transposed   dst[i (in padded to 8)][g·Hp + j] = W_g[j][i]  (B operand of the embedding gradient)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_treelstm_pack(int mode, const bf16_t* __restrict__ w0, const bf16_t* __restrict__ w1,
                                                       const float* __restrict__ b0, const float* __restrict__ b1,
                                                       bf16_t* __restrict__ dst, float* __restrict__ bias, int H,
                                                       int in, int G, long long n) {
  const int Hp = tl_up(H, 8), Hp16 = tl_up(H, 16);
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < n; idx += gridDim.x * 256LL) {
    bf16_t v = 0;
    if (mode == 0) {
      const int Hk = tl_up(H, 32), K = 2 * Hk;
      const int k = (int)(idx % K), j = (int)(idx / K % Hp16), g = (int)(idx / K / Hp16);
      const int s = k >= Hk, kk = k - s * Hk;
      if (j < H && kk < H) v = (s ? w1 : w0)[((long long)g * H + j) * H + kk];
      if (k == 0) bias[g * Hp16 + j] = j < H ? b0[g * H + j] + b1[g * H + j] : 0.f;
    } else if (mode == 1) {
      const int K = tl_up(in, 32);
      const int k = (int)(idx % K), j = (int)(idx / K % Hp16), g = (int)(idx / K / Hp16);
      if (j < H && k < in) v = (g ? w1 : w0)[(long long)j * in + k];
      if (k == 0) bias[g * Hp16 + j] = j < H ? (g ? b1 : b0)[j] : 0.f;
    } else if (mode == 2) {
      const int K = tl_up(G * Hp, 32);
      const int c = (int)(idx % K), k = (int)(idx / K % Hp16), s = (int)(idx / K / Hp16);
      const int g = c / Hp, j = c - g * Hp;
      if (g < G && j < H && k < H) v = (s ? w1 : w0)[((long long)g * H + j) * H + k];
    } else {
      const int K = G * Hp;
      const int c = (int)(idx % K), i = (int)(idx / K);
      const int g = c / Hp, j = c - g * Hp;
      if (j < H && i < in) v = (g ? w1 : w0)[(long long)j * in + i];
    }
    dst[idx] = v;
  }
}

BIGDL_EXPORT int bigdl_treelstm_pack(int mode, const void* w0, const void* w1, const float* b0, const float* b1, void* dst,
                                     float* bias, int H, int in, int G, long long n, hipStream_t s) {
  if (mode < 0 || mode > 3 || !w0 || !dst || H <= 0 || in <= 0 || G < 1 || G > 5 || n <= 0) return (int)hipErrorInvalidValue;
  const int Hp = tl_up(H, 8), Hp16 = tl_up(H, 16);
  const long long want = mode == 0 ? (long long)G * Hp16 * 2 * tl_up(H, 32) : mode == 1 ? (long long)G * Hp16 * tl_up(in, 32)
                         : mode == 2 ? 2LL * Hp16 * tl_up(G * Hp, 32) : (long long)tl_up(in, 8) * G * Hp;
  if (n != want || (mode <= 1 && !(bias && b0)) || (mode != 1 && mode != 3 && !w1) || (mode == 0 && !b1) ||
      ((mode == 1 || mode == 3) && G == 2 && !w1) || (mode == 1 && G == 2 && !b1))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_treelstm_pack, dim3(bigdl_grid(n, 256)), dim3(256), 0, s, mode, (const bf16_t*)w0,
                     (const bf16_t*)w1, b0, b1, (bf16_t*)dst, bias, H, in, G, n);
  return (int)hipGetLastError();
}

// dst[(g·H + j)·ncol + k] += src[(g·Hp + j)·ld + k]: a padded fp32 gradient scratch into the parameter's
// gradient (ncol = 1, ld = 1 for a bias).
__global__ void __launch_bounds__(256) k_treelstm_acc(float* __restrict__ dst, const float* __restrict__ src, int G, int H,
                                                      int Hp, int ncol, int ld) {
  const long long n = (long long)G * H * ncol;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < n; idx += gridDim.x * 256LL) {
    const int k = (int)(idx % ncol), row = (int)(idx / ncol), g = row / H, j = row - g * H;
    dst[idx] += src[((long long)g * Hp + j) * ld + k];
  }
}

BIGDL_EXPORT int bigdl_treelstm_acc(float* dst, const float* src, int G, int H, int ncol, int ld, hipStream_t s) {
  if (!dst || !src || G <= 0 || H <= 0 || ncol <= 0 || ld < ncol) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_treelstm_acc, dim3(bigdl_grid((long long)G * H * ncol, 256)), dim3(256), 0, s, dst, src, G, H,
                     tl_up(H, 8), ncol, ld);
  return (int)hipGetLastError();
}
