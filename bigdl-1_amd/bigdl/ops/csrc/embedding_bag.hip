// Embedding bag (K16): LookupTableSparse.updateOutput / accGradParameters
// (DL/nn/LookupTableSparse.scala:77-208).  A bag of 1-based ids, optional per-id weights, is combined
// into one row: out[b] = Σ_j coef_j · W[id_j − 1], coef_j = ns_j · batchScale_b · w_j, where
// batchScale is 1 (sum), 1/Σw (mean) or 1/sqrt(Σw²) (sqrtn) and ns_j = maxNorm/‖W_r‖ for a row whose
// norm exceeds maxNorm (else 1).  Table T is bf16 or fp32; accumulation and every output are fp32.
//
// Forward, one launch: a group of G lanes owns one bag (G = the smallest power of two ≥ D/V lanes,
// V = 16 bytes of T; 64/G bags per wave).  The bag is the span of `rows` that two binary searches
// find (sorted COO) or the L slots of a dense row (id ≤ 0 = padding).  The group loads G ids and
// weights at once, broadcasts them lane to lane, gathers four rows before the first fma and
// accumulates in list order in registers (a compensated sum): no atomics, no temporaries, the same
// bits for any launch geometry and for both input forms.  With maxNorm the Σx² of the row in registers is reduced
// over the group (xor shuffles).  D > 64·V runs a column loop; there the per-entry scale is
// computed once by a first sweep (which re-reads the row for its norm), written to coef[] and read
// back by the lane that wrote it.
//
// Backward, two launches, no float atomics: the host sorts the ids once (stable); the sorted
// positions after the padding (ids <= 0 sort first) are cut into chunks of 32 and one group of 32 or 64 lanes walks a chunk, accumulating
// each run of equal ids in registers, acc = Σ coef_j · gy[bag_j].  The clip term needs
// Σ_j coef_j ⟨W_r, gy[b_j]⟩ = ⟨W_r, acc⟩, so it is taken from the finished sum: one dot per run, not
// per entry.  A run inside its chunk has a single writer and is added straight to its gradWeight
// row (with several column tiles the unclipped part is added tile by tile while the lanes keep
// their partial dots, then the dot is reduced over the group and a second sweep over the tiles
// subtracts the clip term).  A run that crosses a chunk edge is stored to part[chunk][head|tail][D];
// k_bag_fold, one group per run that crosses an edge, adds its partials in chunk order and
// finishes the row the same way.
#include "common.h"

// No packed-fp32 (v_pk_*_f32) instruction selection in these kernels (see rnn_step.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#define BIGDL_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define BIGDL_NO_PK_F32
#endif

namespace {

constexpr int kChunk = 32;  // sorted positions per backward chunk

struct BagFwd {
  const void* w;          // [n_index, D] table, T
  const void* ids;        // [nnz] 1-based ids (itype)
  const long long* rows;  // [nnz] ascending bag of each entry, or null: fixed stride L
  const float* wts;       // [nnz] or null
  float* out;             // [n, D]
  float* coef;            // [nnz]
  float* inv2;            // [nnz] or null (max_norm <= 0)
  int* err;
  int n, nnz, L, D, G, itype, comb, n_index;
  float max_norm;
};

struct BagBwd {
  float* gw;              // [n_index, D]
  const void* w;          // table, TW (read only for clipped rows)
  const void* gy;         // [n, D], TG
  const void* sid;        // [nnz] sorted ids (itype)
  const long long* perm;  // [nnz] entry of each sorted position
  const long long* rows;  // [nnz] bag of each entry, or null: entry / L
  const float* coef;      // [nnz]
  const float* inv2;      // [nnz] or null
  float* part;            // [nchunk, 2, D]
  int n, nnz, L, D, G, itype, nchunk, n_index;
  float scale;
};

__device__ __forceinline__ long long raw_id(const void* ids, int itype, int i, bool* inexact) {
  if (itype == 0) {
    const float f = ((const float*)ids)[i];
    const long long r = (long long)f;
    *inexact = f != (float)r;
    return r;
  }
  *inexact = false;
  return itype == 1 ? ((const long long*)ids)[i] : (long long)((const int*)ids)[i];
}

// sort key of the backward: the id clamped from above (monotone, so the order holds); <= 0 = skipped
__device__ __forceinline__ int key_at(const void* sid, int itype, int i, int n_index) {
  bool ix;
  const long long r = raw_id(sid, itype, i, &ix);
  return r > n_index ? n_index : (r < 0 ? 0 : (int)r);
}

// first sorted position with a key > 0: padding sorts first, and the chunk grid starts after it, so the
// sums are grouped the same way for a dense input as for the COO input without the padding
__device__ __forceinline__ int first_pos(const void* sid, int itype, int nnz, int n_index) {
  if (key_at(sid, itype, 0, n_index) > 0) return 0;
  int lo = 1, hi = nnz;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (key_at(sid, itype, mid, n_index) <= 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <typename T, int V> struct Row;
template <> struct Row<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float* o) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w;
  }
};
template <> struct Row<float, 1> {
  static __device__ __forceinline__ void ld(const float* p, float* o) { o[0] = p[0]; }
};
template <> struct Row<bf16_t, 8> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* o) { load8(p, o); }
};
template <> struct Row<bf16_t, 4> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* o) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    o[0] = __uint_as_float(u.x << 16); o[1] = __uint_as_float(u.x & 0xFFFF0000u);
    o[2] = __uint_as_float(u.y << 16); o[3] = __uint_as_float(u.y & 0xFFFF0000u);
  }
};
template <> struct Row<bf16_t, 1> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* o) { o[0] = bf2f(p[0]); }
};

template <int V> __device__ __forceinline__ void st_f32(float* p, const float* o) {
  if constexpr (V == 1) {
    p[0] = o[0];
  } else {
#pragma unroll
    for (int v = 0; v < V; v += 4) *reinterpret_cast<float4*>(p + v) = make_float4(o[v], o[v + 1], o[v + 2], o[v + 3]);
  }
}

// sum over the G lanes of a group; every lane gets the same bits (each step adds a commuting pair)
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// first i in [lo, hi) with rows[i] >= b
__device__ __forceinline__ int lower_bound(const long long* rows, int lo, int hi, long long b) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rows[mid] < b) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one lane's entry of the cooperative load: row index (clamped), weight, validity
struct Entry { int r; float w; int ok; };

__device__ __forceinline__ Entry load_entry(const BagFwd& p, int j, bool in_span, bool flag) {
  Entry e = {0, 0.f, 0};
  if (!in_span) return e;
  bool ix;
  const long long raw = raw_id(p.ids, p.itype, j, &ix);
  if (p.rows == nullptr && raw <= 0) return e;  // dense padding
  if (flag && (raw < 1 || raw > p.n_index || ix)) atomicOr(p.err, 1);
  e.r = raw < 1 ? 0 : (raw > p.n_index ? p.n_index - 1 : (int)raw - 1);
  e.w = p.wts != nullptr ? p.wts[j] : 1.f;
  e.ok = 1;
  return e;
}

template <typename T, int V>
__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_bag_fwd(BagFwd p) {
  const int G = p.G, D = p.D;
  const int lig = threadIdx.x & (G - 1);
  const long long bag = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
  if (bag >= p.n) return;
  int lo, hi;
  if (p.rows != nullptr) {
    lo = lower_bound(p.rows, 0, p.nnz, bag);
    hi = lower_bound(p.rows, lo, p.nnz, bag + 1);
  } else {
    lo = (int)bag * p.L;
    hi = lo + p.L;
  }
  const T* __restrict__ W = (const T*)p.w;
  const int ntile = (D + G * V - 1) / (G * V);
  const bool pre = ntile > 1;  // G == 64 then: one bag per wave

  // batch scale: the denominator is accumulated in list order, one entry at a time
  float bs = 1.f;
  if (p.comb != 0) {
    float s = 0.f;
    if (p.rows != nullptr && p.wts == nullptr) {
      s = (float)(hi - lo);
    } else {
      for (int base = lo; base < hi; base += G) {
        const Entry me = load_entry(p, base + lig, base + lig < hi, false);
        const int cnt = min(G, hi - base);
        for (int e = 0; e < cnt; ++e) {
          const float we = __shfl(me.w, e, G);
          if (__shfl(me.ok, e, G)) s += p.comb == 1 ? we : we * we;
        }
      }
    }
    bs = 1.f / fmaxf(p.comb == 1 ? s : sqrtf(s), 1e-12f);
  }

  if (pre) {  // column loop: the complete per-entry scale first, kept in coef[] / inv2[]
    for (int base = lo; base < hi; base += G) {
      const int j = base + lig;
      const Entry me = load_entry(p, j, j < hi, true);
      const int cnt = min(G, hi - base);
      float cme = 0.f, ime = 0.f;
      if (p.max_norm > 0.f) {
        for (int e = 0; e < cnt; ++e) {
          if (!__shfl(me.ok, e, G)) continue;
          const T* src = W + (long long)__shfl(me.r, e, G) * D;
          float ss = 0.f;
          for (int c = lig * V; c < D; c += G * V) {
            float x[V];
            Row<T, V>::ld(src + c, x);
#pragma unroll
            for (int v = 0; v < V; ++v) ss = fmaf(x[v], x[v], ss);
          }
          ss = group_sum(ss, G);
          const float nrm = sqrtf(ss);
          if (lig == e) {
            const bool clip = nrm > p.max_norm;
            cme = (clip ? p.max_norm / nrm : 1.f) * bs * me.w;
            ime = clip ? 1.f / ss : 0.f;
          }
        }
      } else {
        cme = me.ok ? bs * me.w : 0.f;
      }
      if (j < hi) {
        p.coef[j] = cme;
        if (p.inv2 != nullptr) p.inv2[j] = ime;
      }
    }
  }

  for (int t = 0; t < ntile; ++t) {
    const int c = (t * G + lig) * V;
    const bool cin = c < D;
    float acc[V], cmp[V];  // compensated (Kahan) sum: a long bag keeps the accuracy of a short one
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = cmp[v] = 0.f;
    for (int base = lo; base < hi; base += G) {
      const int j = base + lig;
      const Entry me = load_entry(p, j, j < hi, !pre);
      float cme = (pre && j < hi) ? p.coef[j] : 0.f, ime = 0.f;
      const int cnt = min(G, hi - base);
      for (int e0 = 0; e0 < cnt; e0 += 4) {
        float x[4][V], ce[4];
        int ve[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four row gathers in flight
          const int e = min(e0 + u, cnt - 1);  // a source lane inside the group
          ve[u] = (e0 + u < cnt) & __shfl(me.ok, e, G);
          const int r = __shfl(me.r, e, G);
          ce[u] = __shfl(pre ? cme : me.w, e, G);
#pragma unroll
          for (int v = 0; v < V; ++v) x[u][v] = 0.f;
          if (ve[u] && cin) Row<T, V>::ld(W + (long long)r * D + c, x[u]);
        }
        if (!pre) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float ns = 1.f, i2 = 0.f;
            if (p.max_norm > 0.f) {
              float ss = 0.f;
#pragma unroll
              for (int v = 0; v < V; ++v) ss = fmaf(x[u][v], x[u][v], ss);
              ss = group_sum(ss, G);
              const float nrm = sqrtf(ss);
              if (ve[u] && nrm > p.max_norm) {
                ns = p.max_norm / nrm;
                i2 = 1.f / ss;
              }
            }
            ce[u] = ns * bs * ce[u];
            if (ve[u] && lig == e0 + u) {
              cme = ce[u];
              ime = i2;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (ve[u]) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
              const float y = fmaf(ce[u], x[u][v], -cmp[v]);
              const float t = acc[v] + y;
              cmp[v] = (t - acc[v]) - y;
              acc[v] = t;
            }
          }
      }
      if (!pre && j < hi) {
        p.coef[j] = cme;
        if (p.inv2 != nullptr) p.inv2[j] = ime;
      }
    }
    if (cin) st_f32<V>(p.out + bag * D + c, acc);
  }
}

// gw row r (columns of this lane) += scale · (acc − dot · i2 · W_r), the finished sum of one run.
// Single tile: acc and the row are in registers.  Several tiles: the unclipped part was added tile
// by tile; this subtracts the clip term once the dot is complete.
template <typename TW, int V>
__device__ __forceinline__ void finish_row(const BagBwd& p, int r, int lig, int ntile, float i2, float pdot,
                                           const float* acc, const float* wv) {
  const int G = p.G, D = p.D;
  float* __restrict__ dst = p.gw + (long long)r * D;
  const float k = i2 > 0.f ? group_sum(pdot, G) * i2 : 0.f;  // i2 is the same in every lane of the group
  if (ntile == 1) {
    const int c = lig * V;
    if (c < D) {
      float g[V];
      Row<float, V>::ld(dst + c, g);
#pragma unroll
      for (int v = 0; v < V; ++v) g[v] += p.scale * (acc[v] - k * wv[v]);
      st_f32<V>(dst + c, g);
    }
  } else if (i2 > 0.f) {
    const TW* __restrict__ wr = (const TW*)p.w + (long long)r * D;
    for (int c = lig * V; c < D; c += G * V) {
      float g[V], x[V];
      Row<float, V>::ld(dst + c, g);
      Row<TW, V>::ld(wr + c, x);
#pragma unroll
      for (int v = 0; v < V; ++v) g[v] -= p.scale * (k * x[v]);
      st_f32<V>(dst + c, g);
    }
  }
}

// after a tile's sum is known: the partial dot, and (several tiles) the unclipped add
template <typename TW, int V>
__device__ __forceinline__ void tile_done(const BagBwd& p, int r, int c, int ntile, float i2, float* pdot,
                                          const float* acc, float* wv) {
#pragma unroll
  for (int v = 0; v < V; ++v) wv[v] = 0.f;
  if (c >= p.D) return;
  if (i2 > 0.f) {
    Row<TW, V>::ld((const TW*)p.w + (long long)r * p.D + c, wv);
#pragma unroll
    for (int v = 0; v < V; ++v) *pdot = fmaf(wv[v], acc[v], *pdot);
  }
  if (ntile > 1) {
    float* dst = p.gw + (long long)r * p.D + c;
    float g[V];
    Row<float, V>::ld(dst, g);
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] += p.scale * acc[v];
    st_f32<V>(dst, g);
  }
}

template <typename TW, typename TG, int V>
__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_bag_bwd(BagBwd p) {
  const int G = p.G, D = p.D;  // G is 32 or 64: one lane per position of the chunk
  const int lig = threadIdx.x & (G - 1);
  const int q = (int)(((long long)blockIdx.x * 256 + threadIdx.x) / G);
  if (q >= p.nchunk) return;
  const int s0 = first_pos(p.sid, p.itype, p.nnz, p.n_index) + q * kChunk;
  if (s0 >= p.nnz) return;
  const int cnt = min(kChunk, p.nnz - s0);
  const int ntile = (D + G * V - 1) / (G * V);
  const TG* __restrict__ GY = (const TG*)p.gy;

  int mk = 0, mb = 0;
  float mc = 0.f, mi = 0.f;
  if (lig < cnt) {
    mk = key_at(p.sid, p.itype, s0 + lig, p.n_index);
    long long j = p.perm[s0 + lig];
    j = j < 0 ? 0 : (j >= p.nnz ? p.nnz - 1 : j);
    const long long b = p.rows != nullptr ? p.rows[j] : j / p.L;
    mb = (int)(b < 0 ? 0 : (b >= p.n ? p.n - 1 : b));
    mc = p.coef[j];
    mi = p.inv2 != nullptr ? p.inv2[j] : 0.f;
  }
  const int kprev = s0 > 0 ? key_at(p.sid, p.itype, s0 - 1, p.n_index) : -1;
  const int knext = s0 + cnt < p.nnz ? key_at(p.sid, p.itype, s0 + cnt, p.n_index) : -1;

  for (int rs = 0, re; rs < cnt; rs = re) {
    const int ke = __shfl(mk, rs, G);
    re = rs + 1;
    while (re < cnt && __shfl(mk, re, G) == ke) ++re;
    if (ke <= 0) continue;  // padding sorts first
    const bool head = rs == 0 && kprev == ke, tail = re == cnt && knext == ke;
    const bool slab = head || tail;
    const int r = ke - 1;
    const float i2 = slab ? 0.f : __shfl(mi, rs, G);
    float pdot = 0.f, acc[V], wv[V];
    for (int t = 0; t < ntile; ++t) {
      const int c = (t * G + lig) * V;
      const bool cin = c < D;
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = 0.f;
      for (int e0 = rs; e0 < re; e0 += 4) {
        float g[4][V], ce[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four gy rows in flight
          const int e = min(e0 + u, re - 1);
          const int b = __shfl(mb, e, G);
          ce[u] = e0 + u < re ? __shfl(mc, e, G) : 0.f;
#pragma unroll
          for (int v = 0; v < V; ++v) g[u][v] = 0.f;
          if (e0 + u < re && cin) Row<TG, V>::ld(GY + (long long)b * D + c, g[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e0 + u < re) {
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = fmaf(ce[u], g[u][v], acc[v]);
          }
      }
      if (slab) {
        if (cin) st_f32<V>(p.part + ((long long)q * 2 + (head ? 0 : 1)) * D + c, acc);
      } else {
        tile_done<TW, V>(p, r, c, ntile, i2, &pdot, acc, wv);
      }
    }
    if (!slab) finish_row<TW, V>(p, r, lig, ntile, i2, pdot, acc, wv);
  }
}

// One group per chunk edge e (between chunks e and e+1).  The run that crosses it is folded by the
// edge where it starts: tail[e], then head[e+1], head[e+2], ... while the run goes on.
template <typename TW, int V>
__global__ void __launch_bounds__(256) BIGDL_NO_PK_F32 k_bag_fold(BagBwd p) {
  const int G = p.G, D = p.D;
  const int lig = threadIdx.x & (G - 1);
  const int q = (int)(((long long)blockIdx.x * 256 + threadIdx.x) / G);
  if (q >= p.nchunk - 1) return;
  const int p0 = first_pos(p.sid, p.itype, p.nnz, p.n_index);
  const int pos = p0 + (q + 1) * kChunk;  // the start of chunk q+1
  if (pos >= p.nnz) return;
  const int ke = key_at(p.sid, p.itype, pos, p.n_index);
  if (ke <= 0 || key_at(p.sid, p.itype, pos - 1, p.n_index) != ke) return;
  if (q > 0 && key_at(p.sid, p.itype, pos - kChunk - 1, p.n_index) == ke) return;  // started earlier
  const int r = ke - 1;
  float i2 = 0.f;
  if (p.inv2 != nullptr) {
    long long j = p.perm[pos];
    j = j < 0 ? 0 : (j >= p.nnz ? p.nnz - 1 : j);
    i2 = p.inv2[j];
  }
  // the run ends before the first larger key (binary search: a heavy hitter spans hundreds of chunks);
  // it reaches the first position of every chunk up to mlast, so each of them stored a head partial
  int lo = pos + 1, hi = p.nnz;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (key_at(p.sid, p.itype, mid, p.n_index) <= ke) lo = mid + 1; else hi = mid;
  }
  const int mlast = (lo - 1 - p0) / kChunk;
  const int ntile = (D + G * V - 1) / (G * V);
  float pdot = 0.f, acc[V], wv[V];
  for (int t = 0; t < ntile; ++t) {
    const int c = (t * G + lig) * V;
    const bool cin = c < D;
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    if (cin) Row<float, V>::ld(p.part + ((long long)q * 2 + 1) * D + c, acc);
#pragma unroll 4
    for (int m = q + 1; m <= mlast; ++m) {  // independent loads, added in chunk order
      if (cin) {
        float h[V];
        Row<float, V>::ld(p.part + (long long)m * 2 * D + c, h);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += h[v];
      }
    }
    tile_done<TW, V>(p, r, c, ntile, i2, &pdot, acc, wv);
  }
  finish_row<TW, V>(p, r, lig, ntile, i2, pdot, acc, wv);
}

int group_lanes(int D, int V, int lo) {
  const int need = (D + V - 1) / V;
  int g = lo;
  while (g < 64 && g < need) g <<= 1;
  return g;
}

template <typename TW, typename TG, int V>
void launch_bwd(const BagBwd& p, hipStream_t s) {
  const long long per = 256 / p.G;
  hipLaunchKernelGGL((k_bag_bwd<TW, TG, V>), dim3((unsigned)((p.nchunk + per - 1) / per)), dim3(256), 0, s, p);
  if (p.nchunk > 1)
    hipLaunchKernelGGL((k_bag_fold<TW, V>), dim3((unsigned)((p.nchunk - 1 + per - 1) / per)), dim3(256), 0, s, p);
}

}  // namespace

// itype: 0 = float32 ids, 1 = int64, 2 = int32; dtype: 0 = bf16 table, 1 = fp32;
// comb: 0 = sum, 1 = mean, 2 = sqrtn; rows null = fixed stride L (nnz = n·L)
BIGDL_EXPORT int bigdl_embedding_bag_fwd(const void* w, const void* ids, int itype, const long long* rows,
                                         const float* wts, float* out, float* coef, float* inv2, long long n,
                                         long long nnz, long long L, long long n_index, int D, int dtype, int comb,
                                         float max_norm, int* err, hipStream_t s) {
  if (n <= 0 || nnz < 0 || n >= (1LL << 31) || nnz >= (1LL << 31) || n_index <= 0 || n_index >= (1LL << 31) || D < 1)
    return (int)hipErrorInvalidValue;
  if (itype < 0 || itype > 2 || comb < 0 || comb > 2 || dtype < 0 || dtype > 1) return (int)hipErrorInvalidValue;
  if (rows == nullptr && (L < 0 || n * L != nnz)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)w & 15) || ((uintptr_t)out & 15) || ((uintptr_t)err & 3) || err == nullptr || coef == nullptr)
    return (int)hipErrorInvalidValue;
  if (max_norm > 0.f && inv2 == nullptr) return (int)hipErrorInvalidValue;
  BagFwd p = {w, ids, rows, wts, out, coef, max_norm > 0.f ? inv2 : nullptr, err, (int)n, (int)nnz, (int)L, D, 1,
              itype, comb, (int)n_index, max_norm};
  const int V = dtype == 0 ? 8 : 4;
  const bool vec = D % V == 0;
  p.G = group_lanes(D, vec ? V : 1, 1);
  const long long per = 256 / p.G;
  const dim3 g((unsigned)((n + per - 1) / per));
  if (dtype == 0) {
    if (vec) hipLaunchKernelGGL((k_bag_fwd<bf16_t, 8>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_bag_fwd<bf16_t, 1>), g, dim3(256), 0, s, p);
  } else {
    if (vec) hipLaunchKernelGGL((k_bag_fwd<float, 4>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_bag_fwd<float, 1>), g, dim3(256), 0, s, p);
  }
  BIGDL_CHECK_LAUNCH();
}

// part: [ceil(nnz / 32), 2, D] floats of scratch (written before it is read); gdtype: gy's dtype
BIGDL_EXPORT int bigdl_embedding_bag_bwd(float* gw, const void* w, int dtype, const void* gy, int gdtype,
                                         const void* sid, int itype, const long long* perm, const long long* rows,
                                         const float* coef, const float* inv2, float* part, long long n, long long nnz,
                                         long long L, long long n_index, int D, float scale, hipStream_t s) {
  if (n <= 0 || nnz <= 0 || n >= (1LL << 31) || nnz >= (1LL << 31) || n_index <= 0 || n_index >= (1LL << 31) || D < 1)
    return (int)hipErrorInvalidValue;
  if (itype < 0 || itype > 2 || dtype < 0 || dtype > 1 || gdtype < 0 || gdtype > 1) return (int)hipErrorInvalidValue;
  if (rows == nullptr && (L <= 0 || n * L != nnz)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)w & 15) || ((uintptr_t)gw & 15) || ((uintptr_t)gy & 15) || ((uintptr_t)part & 15))
    return (int)hipErrorInvalidValue;
  if (gw == nullptr || perm == nullptr || coef == nullptr || part == nullptr) return (int)hipErrorInvalidValue;
  BagBwd p = {gw, w, gy, sid, perm, rows, coef, inv2, part, (int)n, (int)nnz, (int)L, D, 32, itype,
              (int)((nnz + kChunk - 1) / kChunk), (int)n_index, scale};
  const bool vec = D % 4 == 0;
  p.G = group_lanes(D, vec ? 4 : 1, 32);
  if (dtype == 0) {
    if (gdtype == 0) { if (vec) launch_bwd<bf16_t, bf16_t, 4>(p, s); else launch_bwd<bf16_t, bf16_t, 1>(p, s); }
    else { if (vec) launch_bwd<bf16_t, float, 4>(p, s); else launch_bwd<bf16_t, float, 1>(p, s); }
  } else {
    if (gdtype == 0) { if (vec) launch_bwd<float, bf16_t, 4>(p, s); else launch_bwd<float, bf16_t, 1>(p, s); }
    else { if (vec) launch_bwd<float, float, 4>(p, s); else launch_bwd<float, float, 1>(p, s); }
  }
  BIGDL_CHECK_LAUNCH();
}
