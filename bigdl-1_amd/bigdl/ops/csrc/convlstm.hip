// ConvLSTMPeephole recurrence (DL/nn/ConvLSTMPeephole.scala:93-230): one launch per time step, forward
// and BPTT.  The recurrent convolution h_{t-1} ⊛ Wh_k is an implicit GEMM on mfma_f32_16x16x32_bf16 and
// the gate / cell / peephole math runs on its accumulators, so no pre-activation ever reaches memory.
//
// Layout.  Everything is pixel-major NHWC and time-major: the hidden sequence [T+1][B][H][W][C] bf16
// (slot 0 = h0, so step t reads slot t and writes slot t+1, and slots 0..T-1 are the weight gradient's
// activation batch with no copy), gx / DG [T][B][H][W][4C] bf16, c / tanh c [T][B][H][W][C] and the four
// activations [T][B][H][W][4C] fp32.  Gate blocks are (i, f, o, g), the order of the layer's gx / gh
// lists; peephole rows (p_i, p_f, p_o), p_i and p_f on c_{t-1}, p_o on c_t.
//
// Work split.  A block of 4 waves owns an 8×8 pixel tile of one image.  A 16-pixel MFMA operand is two
// tile rows of 8 pixels.  The weights are the MFMA "A" side (16 output channels × 32 reduction
// indices), the pixels the "B" side, so a lane ends up with 4 consecutive channels of ONE pixel.
//   forward  (M = B·H·W, N = 4C, K = kC²·C): gate-interleaved N — a wave's four accumulator tiles are
//            the gates i, f, o, g of the same 16 hidden channels, read through four weight pointers
//            where the layer's parameters lie ([C][kC][kC][C], the conv layers' physical layout).  The
//            cell update therefore needs no exchange between lanes.  Block = 32 channels × 4 gates =
//            128 columns; wave w takes channels 16·(w & 1) and pixel rows 4·(w >> 1) .. +3.
//   backward (N = C, K = kC²·4C): dh = gy + Σ_k DG_{t+1,k} ⊛ flip(Wh_k)ᵀ.  The reduction runs gate block
//            by gate block (4 segments of the forward's shape, each with its own transformed weight
//            [C_in][kC][kC][C_out], flipped and transposed once per sequence), so the halo in LDS is C
//            channels wide as in the forward, not 4C.  Block = 64 channels; wave w takes channels 16·w
//            and all 64 pixels.
//
// Halo staging.  The tile's (8 + kC − 1)² × C halo of the reduction operand is staged in LDS once (per
// segment); every tap's B fragment is a ds_read_b128 from it at a shifted address.  Pixels outside the
// image are stored as zeros, so border taps need no predicate in the loop.  In 16-byte units the
// pixel pitch s = C/8 made odd and the halo row pitch R ≡ 8 (mod 16): the 16 lanes of a fragment's lane
// group (2 rows × 8 pixels, same channel chunk) sit at 8·row + s·col (mod 16) — sixteen different
// 16-byte slots of the 256-byte bank period — and a tap shift adds the same constant to all of them,
// so the reads stay conflict-free under every shift.
//
// Weight streaming.  Per (tap, 64-channel chunk) the block's columns × 64 reduction indices are one
// stage of a two-stage LDS ring (column pitch 9 units, odd): the next stage's global loads are issued
// before the current stage's MFMAs and stored after them; one __syncthreads() per stage hands the ring
// over (a raw s_barrier does not drain ds_writes on gfx950).  The forward's epilogue operands (the
// gx tile, c_{t-1}, the peephole rows) are loaded before the loop, under the MFMAs.  The backward's 30
// floats per (pixel, quad) × 4 pixel tiles would not fit in registers next to the accumulators; they
// are read in the epilogue.
//
// Partly filled K: C % 8 == 0; a 32-index MFMA step past C takes zero fragments on both sides.
// LDS bytes (bigdl_convlstm_lds_bytes) must stay within 64 KB; the Python eligibility check asks the
// same function.
#include "common.h"

typedef short v8s __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

#if defined(__HIP_DEVICE_COMPILE__)
#define BIGDL_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define BIGDL_NO_PK_F32
#endif

struct ConvLstmP {
  const bf16_t* a;     // reduction operand images [B][H][W][lda]: h_{t-1} (lda = C) / DG_{t+1} (lda = 4C); null = 0
  const bf16_t* w[4];  // forward: Wh_i, Wh_f, Wh_o, Wh_g [C][kC²][C]; backward: w[0] = the transformed blocks [4][C][kC²][C]
  int B, H, W, C, kC;
  const bf16_t* gx;     // forward: input-conv pre-activations [B][H][W][4C]
  const float* c_prev;  // [B][H][W][C] (null = 0)
  const float* peep;    // [3][C] (null = no peephole)
  bf16_t* h_out;        // forward: h_t [B][H][W][C]
  float* c_out;         // forward: c_t (training save or inference ping-pong)
  float* act;           // fwd out / bwd in: i, f, o, g [B][H][W][4C] (bwd: null = plain dh to dc_prev)
  float* tc;            // fwd out / bwd in: tanh c_t
  const bf16_t* gy;     // backward: output gradient of this step [B][H][W][C]
  const float* dc_next; // backward: dc from step t+1 (null = 0)
  bf16_t* dg;           // backward: DG_t [B][H][W][4C]
  float* dc_prev;       // backward: dc_{t-1} [B][H][W][C]
};

constexpr int kTile = 8;       // pixel tile edge
constexpr int kColPitch = 9;   // ring column pitch, 16-byte units (8 + 1)

__host__ __device__ inline int cl_pix_pitch(int C) { return (C >> 3) | 1; }
__host__ __device__ inline int cl_row_pitch(int hw, int s) {
  const int r = hw * s;
  return r + ((8 - r % 16) + 16) % 16;
}

__device__ __forceinline__ float cl_sgm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ void cl_ldb4(const bf16_t* p, float* o) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  o[0] = __uint_as_float(v.x << 16);
  o[1] = __uint_as_float(v.x & 0xFFFF0000u);
  o[2] = __uint_as_float(v.y << 16);
  o[3] = __uint_as_float(v.y & 0xFFFF0000u);
}
__device__ __forceinline__ void cl_ldf4(const float* p, float* o) {
  if (!p) { o[0] = o[1] = o[2] = o[3] = 0.f; return; }
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void cl_stf4(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void cl_stb4(bf16_t* p, const float* v) {
  *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                                            (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16));
}

// 16-byte piece `i` of a thread's share of ring stage `st`: column (tid >> 3) + 32·i, unit tid & 7.  A forward
// column is (gate i, channel tid >> 3) and reads that gate's own weight `w`; a backward column is a channel.
template <int MODE>
__device__ __forceinline__ bigdl_u32x4 cl_wload(const bf16_t* w, int j0, int tid, int i, int st, int nch, int taps, int C) {
  const int tap = st / nch, c = ((st % nch) << 6) + (tid & 7) * 8;
  const int j = j0 + (tid >> 3) + (MODE == 0 ? 0 : i * 32);
  if (j < C && c < C) return *reinterpret_cast<const bigdl_u32x4*>(w + ((long long)j * taps + tap) * C + c);
  return bigdl_u32x4{0u, 0u, 0u, 0u};
}

// MODE 0 forward (4 gates × 32 channels per block), MODE 1 backward (64 channels, 4 gate segments)
template <int MODE>
__device__ __forceinline__ void convlstm_body(const ConvLstmP& p) {
  constexpr int G = MODE == 0 ? 4 : 1;      // accumulator tiles per (wave, pixel tile)
  constexpr int NCS = MODE == 0 ? 2 : 4;    // 16-channel groups per block
  constexpr int NPQ = MODE == 0 ? 2 : 4;    // 16-pixel tiles per wave
  constexpr int NSEG = MODE == 0 ? 1 : 4;   // reduction segments (backward: one per gate block)
  constexpr int NCOL = NCS * 16 * G;        // weight columns per ring stage
  constexpr int NLD = NCOL * 8 / 256;       // 16-byte weight loads per thread and stage
  extern __shared__ __attribute__((aligned(16))) bigdl_u32x4 cl_lds[];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int C = p.C, kC = p.kC, taps = kC * kC, P = kC >> 1;
  const int hw = kTile + kC - 1, cu = C >> 3, s = cl_pix_pitch(C), Rp = cl_row_pitch(hw, s);
  bigdl_u32x4* halo = cl_lds;
  bigdl_u32x4* ring = cl_lds + hw * Rp;
  const int tiles_x = (p.W + kTile - 1) / kTile;
  const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
  const int b = blockIdx.z, j0 = blockIdx.y * NCS * 16;
  const int csub = wid % NCS, pq0 = (wid / NCS) * NPQ;
  const int ch = j0 + csub * 16 + fq * 4;   // this lane's channel quad (C % 4 == 0: all in or all out)
  const bool chv = ch < C;
  const int px = fr & 7, pr = fr >> 3;      // pixel of the lane inside a 16-pixel tile: row pr, column px
  const int lda = MODE == 0 ? C : 4 * C;

  long long pix[NPQ];
  bool pv[NPQ];
#pragma unroll
  for (int q = 0; q < NPQ; ++q) {
    const int y = ty0 + 2 * (pq0 + q) + pr, x = tx0 + px;
    pv[q] = chv && y < p.H && x < p.W;
    pix[q] = ((long long)b * p.H + y) * p.W + x;
  }

  // forward: epilogue operands in flight under the MFMA loop
  float pre_gx[MODE == 0 ? NPQ : 1][4][4], pre_c[MODE == 0 ? NPQ : 1][4], pp[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k) cl_ldf4((p.peep && chv) ? p.peep + k * C + ch : nullptr, pp[k]);
  if constexpr (MODE == 0) {
#pragma unroll
    for (int q = 0; q < NPQ; ++q) {
      if (!pv[q]) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) cl_ldb4(p.gx + pix[q] * 4 * C + g * C + ch, pre_gx[q][g]);
      cl_ldf4(p.c_prev ? p.c_prev + pix[q] * C + ch : nullptr, pre_c[q]);
    }
  }

  v4f acc[NPQ][G];
#pragma unroll
  for (int q = 0; q < NPQ; ++q)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[q][g] = v4f{0.f, 0.f, 0.f, 0.f};

  if (p.a) {
    const int nch = (C + 63) >> 6, S = taps * nch;
    const bigdl_u32x4 z4 = bigdl_u32x4{0u, 0u, 0u, 0u};
    for (int seg = 0; seg < NSEG; ++seg) {
      // halo of this segment's C channels: zeros outside the image
      const int nh = hw * hw * cu;
      for (int idx = tid; idx < nh; idx += 256) {
        const int u = idx % cu, hp = idx / cu, hx = hp % hw, hy = hp / hw;
        const int y = ty0 - P + hy, x = tx0 - P + hx;
        bigdl_u32x4 v = z4;
        if (y >= 0 && y < p.H && x >= 0 && x < p.W)
          v = *reinterpret_cast<const bigdl_u32x4*>(p.a + (((long long)b * p.H + y) * p.W + x) * lda + seg * C + u * 8);
        halo[hy * Rp + hx * s + u] = v;
      }
      bigdl_u32x4 wr[NLD];
      const bf16_t* wseg = MODE == 0 ? nullptr : p.w[0] + (long long)seg * C * taps * C;
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        wr[i] = cl_wload<MODE>(MODE == 0 ? p.w[i & 3] : wseg, j0, tid, i, 0, nch, taps, C);
        ring[((tid >> 3) + i * 32) * kColPitch + (tid & 7)] = wr[i];
      }
      __syncthreads();
      for (int st = 0; st < S; ++st) {
        if (st + 1 < S) {
#pragma unroll
          for (int i = 0; i < NLD; ++i)
            wr[i] = cl_wload<MODE>(MODE == 0 ? p.w[i & 3] : wseg, j0, tid, i, st + 1, nch, taps, C);
        }
        const int tap = st / nch, c0 = (st % nch) << 6, ty = tap / kC, tx = tap % kC;
        const bigdl_u32x4* wb = ring + (st & 1) * NCOL * kColPitch;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          if (c0 + ks * 32 >= C) break;
          const int cun = (c0 >> 3) + ks * 4 + fq;
          v8s xf[NPQ];
#pragma unroll
          for (int q = 0; q < NPQ; ++q) {
            const bigdl_u32x4 v = cun < cu ? halo[(2 * (pq0 + q) + pr + ty) * Rp + (px + tx) * s + cun] : z4;
            xf[q] = __builtin_bit_cast(v8s, v);
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const v8s wf = __builtin_bit_cast(v8s, wb[((g * NCS + csub) * 16 + fr) * kColPitch + ks * 4 + fq]);
#pragma unroll
            for (int q = 0; q < NPQ; ++q) acc[q][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[q], acc[q][g], 0, 0, 0);
          }
        }
        if (st + 1 < S) {
#pragma unroll
          for (int i = 0; i < NLD; ++i)
            ring[(((st + 1) & 1) * NCOL + (tid >> 3) + i * 32) * kColPitch + (tid & 7)] = wr[i];
        }
        __syncthreads();
      }
    }
  }

#pragma unroll
  for (int q = 0; q < NPQ; ++q) {
    if (!pv[q]) continue;
    const long long o1 = pix[q] * C + ch, o4 = pix[q] * 4 * C + ch;
    if constexpr (MODE == 0) {
      float gi[4], gf[4], go[4], gg[4], c[4], tcv[4], h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float cp = pre_c[q][e];
        gi[e] = cl_sgm(pre_gx[q][0][e] + acc[q][0][e] + pp[0][e] * cp);
        gf[e] = cl_sgm(pre_gx[q][1][e] + acc[q][1][e] + pp[1][e] * cp);
        gg[e] = tanhf(pre_gx[q][3][e] + acc[q][3][e]);
        c[e] = gf[e] * cp + gi[e] * gg[e];
        go[e] = cl_sgm(pre_gx[q][2][e] + acc[q][2][e] + pp[2][e] * c[e]);
        tcv[e] = tanhf(c[e]);
        h[e] = go[e] * tcv[e];
      }
      cl_stb4(p.h_out + o1, h);
      if (p.c_out) cl_stf4(p.c_out + o1, c);
      if (p.act) {
        cl_stf4(p.act + o4, gi);
        cl_stf4(p.act + o4 + C, gf);
        cl_stf4(p.act + o4 + 2 * C, go);
        cl_stf4(p.act + o4 + 3 * C, gg);
      }
      if (p.tc) cl_stf4(p.tc + o1, tcv);
    } else {
      float dh[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) dh[e] = acc[q][0][e];
      if (!p.act) {  // plain product (the initial hidden state's gradient)
        cl_stf4(p.dc_prev + o1, dh);
        continue;
      }
      float gy[4], ai[4], af[4], ao[4], ag[4], tcv[4], cp[4], dn[4];
      cl_ldb4(p.gy + o1, gy);
      cl_ldf4(p.act + o4, ai);
      cl_ldf4(p.act + o4 + C, af);
      cl_ldf4(p.act + o4 + 2 * C, ao);
      cl_ldf4(p.act + o4 + 3 * C, ag);
      cl_ldf4(p.tc + o1, tcv);
      cl_ldf4(p.c_prev ? p.c_prev + o1 : nullptr, cp);
      cl_ldf4(p.dc_next ? p.dc_next + o1 : nullptr, dn);
      float di[4], df[4], dout[4], dgg[4], dcp[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float i = ai[e], f = af[e], o = ao[e], g = ag[e], t = tcv[e];
        const float d_h = gy[e] + dh[e];
        dout[e] = d_h * t * o * (1.f - o);
        const float dc = d_h * o * (1.f - t * t) + dn[e] + dout[e] * pp[2][e];
        di[e] = dc * g * i * (1.f - i);
        df[e] = dc * cp[e] * f * (1.f - f);
        dgg[e] = dc * i * (1.f - g * g);
        dcp[e] = dc * f + di[e] * pp[0][e] + df[e] * pp[1][e];
      }
      cl_stb4(p.dg + o4, di);
      cl_stb4(p.dg + o4 + C, df);
      cl_stb4(p.dg + o4 + 2 * C, dout);
      cl_stb4(p.dg + o4 + 3 * C, dgg);
      cl_stf4(p.dc_prev + o1, dcp);
    }
  }
}

__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_convlstm_fwd(ConvLstmP p) { convlstm_body<0>(p); }
__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_convlstm_bwd(ConvLstmP p) { convlstm_body<1>(p); }

static inline bool cl_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static long long cl_lds_bytes(int mode, int C, int kC) {
  const int hw = kTile + kC - 1;
  const long long halo = (long long)hw * cl_row_pitch(hw, cl_pix_pitch(C));
  const long long ring = 2LL * (mode == 0 ? 128 : 64) * kColPitch;
  return (halo + ring) * 16;
}

// LDS bytes of the larger of the two step kernels: a cell is served when this is ≤ 65536
BIGDL_EXPORT long long bigdl_convlstm_lds_bytes(int C, int kC) {
  if (C <= 0 || C % 8 || kC <= 0 || kC % 2 == 0 || kC > 15) return -1;
  return cl_lds_bytes(0, C, kC);
}

static int cl_launch(int mode, const ConvLstmP& p, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0 || p.W <= 0 || p.B > 65535 || bigdl_convlstm_lds_bytes(p.C, p.kC) < 0)
    return (int)hipErrorInvalidValue;
  const long long lds = cl_lds_bytes(mode, p.C, p.kC);
  if (lds > 65536) return (int)hipErrorInvalidValue;
  const void* ptrs[] = {p.a, p.w[0], p.w[1], p.w[2], p.w[3], p.gx, p.c_prev, p.peep, p.h_out, p.c_out, p.act,
                        p.tc, p.gy, p.dc_next, p.dg, p.dc_prev};
  for (const void* q : ptrs)
    if (!cl_a16(q)) return (int)hipErrorInvalidValue;
  if (mode == 0 ? !(p.gx && p.h_out) : !(p.dc_prev && (!p.act || (p.gy && p.tc && p.dg)))) return (int)hipErrorInvalidValue;
  if (p.a && !(p.w[0] && (mode == 1 || (p.w[1] && p.w[2] && p.w[3])))) return (int)hipErrorInvalidValue;
  const long long tiles = (long long)((p.H + kTile - 1) / kTile) * ((p.W + kTile - 1) / kTile);
  if (tiles > 0x7fffffff) return (int)hipErrorInvalidValue;
  const int cpb = mode == 0 ? 32 : 64;
  const dim3 grid((unsigned)tiles, (unsigned)((p.C + cpb - 1) / cpb), (unsigned)p.B);
  if (mode == 0) hipLaunchKernelGGL(k_convlstm_fwd, grid, dim3(256), (size_t)lds, s, p);
  else hipLaunchKernelGGL(k_convlstm_bwd, grid, dim3(256), (size_t)lds, s, p);
  return (int)hipGetLastError();
}

// One step (mode 0 forward, 1 backward: w0 = the transformed blocks, w1..3 unused); every tensor is the
// dense [B][H][W][·] slice of its step.
BIGDL_EXPORT int bigdl_convlstm_step(int mode, const void* a, const void* w0, const void* w1, const void* w2,
                                     const void* w3, const void* gx, const float* c_prev, const float* peep,
                                     void* h_out, float* c_out, float* act, float* tc, const void* gy,
                                     const float* dc_next, void* dg, float* dc_prev, int B, int H, int W, int C,
                                     int kC, hipStream_t s) {
  if (mode != 0 && mode != 1) return (int)hipErrorInvalidValue;
  ConvLstmP p{};
  p.a = (const bf16_t*)a;
  p.w[0] = (const bf16_t*)w0; p.w[1] = (const bf16_t*)w1; p.w[2] = (const bf16_t*)w2; p.w[3] = (const bf16_t*)w3;
  p.B = B; p.H = H; p.W = W; p.C = C; p.kC = kC;
  p.gx = (const bf16_t*)gx; p.c_prev = c_prev; p.peep = peep; p.h_out = (bf16_t*)h_out; p.c_out = c_out;
  p.act = act; p.tc = tc; p.gy = (const bf16_t*)gy; p.dc_next = dc_next; p.dg = (bf16_t*)dg; p.dc_prev = dc_prev;
  return cl_launch(mode, p, s);
}

// Whole sequence, forward.  hs [T+1][B][H][W][C] with h0 in slot 0; gx [T][B][H][W][4C]; training saves
// cs / tcs [T][..][C] and acts [T][..][4C]; inference (cs null) ping-pongs c through cbuf [2][..][C].
BIGDL_EXPORT int bigdl_convlstm_seq_fwd(void* hs, const void* gx, const float* c0, const void* w0, const void* w1,
                                        const void* w2, const void* w3, const float* peep, float* cs, float* acts,
                                        float* tcs, float* cbuf, int B, int T, int H, int W, int C, int kC,
                                        hipStream_t s) {
  if (T <= 0 || !hs || !gx || !(cs ? (acts && tcs) : cbuf != nullptr)) return (int)hipErrorInvalidValue;
  const long long n1 = (long long)B * H * W * C;
  for (int t = 0; t < T; ++t) {
    float* cprev = t == 0 ? nullptr : (cs ? cs + (t - 1) * n1 : cbuf + ((t - 1) & 1) * n1);
    const int rc = bigdl_convlstm_step(0, (bf16_t*)hs + t * n1, w0, w1, w2, w3, (const bf16_t*)gx + t * 4 * n1,
                                       t == 0 ? c0 : cprev, peep, (bf16_t*)hs + (t + 1) * n1,
                                       cs ? cs + t * n1 : cbuf + (t & 1) * n1, acts ? acts + t * 4 * n1 : nullptr,
                                       tcs ? tcs + t * n1 : nullptr, nullptr, nullptr, nullptr, nullptr, B, H, W, C,
                                       kC, s);
    if (rc) return rc;
  }
  return 0;
}

// Whole sequence, BPTT.  gy [T][..][C]; wt [4][C][kC²][C] the transformed gate blocks; DG [T][..][4C] out; gc [..][C]
// ← dc before the first step (updated in place: every element is read and written by one lane); dh0
// (optional, fp32 [..][C]) ← DG_0 ⊛ flip(Wh)ᵀ, the initial hidden state's gradient.
BIGDL_EXPORT int bigdl_convlstm_seq_bwd(const void* gy, const void* wt, const float* peep, float* acts, float* tcs, const float* cs,
                                        const float* c0, void* DG, float* gc, float* dh0, int B, int T, int H, int W,
                                        int C, int kC, hipStream_t s) {
  if (T <= 0 || !gy || !acts || !tcs || !cs || !DG || !gc) return (int)hipErrorInvalidValue;
  const long long n1 = (long long)B * H * W * C;
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t + 1 == T;
    const int rc = bigdl_convlstm_step(1, last ? nullptr : (bf16_t*)DG + (t + 1) * 4 * n1, wt, nullptr, nullptr, nullptr, nullptr,
                                       t ? cs + (t - 1) * n1 : c0, peep, nullptr, nullptr, acts + t * 4 * n1,
                                       tcs + t * n1, (const bf16_t*)gy + t * n1, last ? nullptr : gc,
                                       (bf16_t*)DG + t * 4 * n1, gc, B, H, W, C, kC, s);
    if (rc) return rc;
  }
  if (dh0)
    return bigdl_convlstm_step(1, DG, wt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, dh0, B, H, W, C, kC, s);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Peephole gradients over pixel rows: per channel j, with n = T·B·H·W rows in time-major order,
//   gp_i[j] += s·Σ DG_i·c_{t-1}   gp_f[j] += s·Σ DG_f·c_{t-1}   gp_o[j] += s·Σ DG_o·c_t
// (DG blocks i, f, o, g; c_{t-1} of row r is row r − B·H·W of cs, or c0 for the first step).  The dense
// cell's kernel (rnn_step.hip) assumes (b, t) row order and the (i, f, g, o) blocks, so this is its
// pixel-row variant: 32 column lanes × 8 channels, 8 row lanes over a 256-row chunk, LDS fold in lane
// order, then one fold of the chunk partials in index order.  No atomics: the same bits on every run.
// ------------------------------------------------------------------------------------------------
constexpr int kCpRows = 256;
constexpr int kCpCols = 256;

__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_convlstm_peep_partial(
    const bf16_t* __restrict__ DG, const float* __restrict__ cs, const float* __restrict__ c0, float* __restrict__ part,
    long long n, long long np, int C) {
  __shared__ float red[7][3][kCpCols];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int j = blockIdx.y * kCpCols + cl * 8;
  const long long r0 = (long long)blockIdx.x * kCpRows;
  float acc[3][8];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  if (j < C) {
    for (int k = rl; k < kCpRows; k += 8) {
      const long long r = r0 + k;
      if (r >= n) break;
      float di[8], df[8], dout[8], cp[8], cc[8];
      load8(DG + r * 4 * C + j, di);
      load8(DG + r * 4 * C + C + j, df);
      load8(DG + r * 4 * C + 2 * C + j, dout);
      const float* pc = r >= np ? cs + (r - np) * C + j : (c0 ? c0 + r * C + j : nullptr);
      cl_ldf4(pc, cp);
      cl_ldf4(pc ? pc + 4 : nullptr, cp + 4);
      cl_ldf4(cs + r * C + j, cc);
      cl_ldf4(cs + r * C + j + 4, cc + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[0][e] += di[e] * cp[e];
        acc[1][e] += df[e] * cp[e];
        acc[2][e] += dout[e] * cc[e];
      }
    }
  }
  if (rl > 0) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[rl - 1][g][cl * 8 + e] = acc[g][e];
  }
  __syncthreads();
  if (rl > 0 || j >= C) return;
#pragma unroll
  for (int w = 0; w < 7; ++w)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] += red[w][g][cl * 8 + e];
  float* o = part + (long long)blockIdx.x * 3 * C + j;  // part [chunks][3][C]
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    cl_stf4(o + (long long)g * C, acc[g]);
    cl_stf4(o + (long long)g * C + 4, acc[g] + 4);
  }
}

__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_convlstm_peep_fold(const float* __restrict__ part, int chunks,
                                                                            float* gp, float scale, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * C) return;
  float a = 0.f;
  for (int c = 0; c < chunks; ++c) a += part[(long long)c * 3 * C + i];
  gp[i] += scale * a;
}

// gp fp32 [3][C] (p_i, p_f, p_o rows) accumulates; part: ⌈n / 256⌉·3·C floats of workspace
BIGDL_EXPORT int bigdl_convlstm_peephole_grad(const void* DG, const float* cs, const float* c0, float* gp, float scale,
                                              float* part, long long npart, long long n, long long np, int C,
                                              hipStream_t s) {
  if (n <= 0 || np <= 0 || n % np || C <= 0 || C % 8 || !DG || !cs || !gp || !part) return (int)hipErrorInvalidValue;
  if (!cl_a16(DG) || !cl_a16(cs) || !cl_a16(c0) || !cl_a16(part)) return (int)hipErrorInvalidValue;
  const long long chunks = (n + kCpRows - 1) / kCpRows;
  if (chunks > 0x7fffffff || npart < chunks * 3 * C) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_convlstm_peep_partial, dim3((unsigned)chunks, (unsigned)((C + kCpCols - 1) / kCpCols)),
                     dim3(256), 0, s, (const bf16_t*)DG, cs, c0, part, n, np, C);
  hipLaunchKernelGGL(k_convlstm_peep_fold, dim3((unsigned)((3 * C + 255) / 256)), dim3(256), 0, s, (const float*)part,
                     (int)chunks, gp, scale, C);
  BIGDL_CHECK_LAUNCH();
}
