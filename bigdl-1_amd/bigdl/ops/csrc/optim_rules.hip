// Fused updates of every elementwise optimisation method but SGD and LARS: Adam, Adagrad, RMSprop,
// Adadelta, Adamax and Ftrl.
//
// ONE streaming kernel (k_optim), templated on an update rule and on the gradient type: grid-stride
// float4 body, the n & 3 tail on block 0, long long indices, a bf16 gradient (the DistriOptimizer's
// reduce-scatter wire shard) widened on load, and the optional bf16 shadow written from the new
// weight as one 8-B store.  HBM-bound: 16 B per lane per access, grid capped at 2048 blocks of 256
// (cdna_hip_programming.md Guideline 11).
//
// k_optim_clip is the same pass with a GradClip operand (optim_common.h): the gradient is clamped and
// L2-scaled right after the load, and the rule runs with scale 1.  k_optim itself is unchanged by it.
//
// A rule is a struct of its hyper-parameters (by value in the kernel arguments) with
//   NS                     number of fp32 state tensors (1 or 2)
//   prepare()              called once per thread on the kernel's copy before the loop: Adam and
//                          Adagrad form their step size here from an iteration count on the device
//                          (the replay-safe form for HIP-graph capture); empty otherwise
//   step(w, g, a, b)       the per-element update over the weight, the raw gradient and the states
// Every rule is the torch form of its class in optim/optim_method.py (the CPU path and the
// oracle), term for term; constants such as 1 - decay are formed on the host in double, as the
// torch form does.  Plain IEEE division and sqrtf only: Adamax's default eps = 1e-38 is a subnormal
// fp32 and must survive (no fast-math, no reciprocal approximations).
#include "optim_common.h"

// ------------------------------------------------------------------------------------------------
// rules
// ------------------------------------------------------------------------------------------------
// RMSprop (DL/optim/RMSprop.scala): s = dr·s + (1-dr)·g'² ; w -= clr·g' / (sqrt(s) + eps)
struct RmspropRule {
  static constexpr int NS = 1;
  float scale, clr, dr, omdr, eps;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void step(float& w, float g, float& s, float&) const {
    const float gg = g * scale;
    s = dr * s + omdr * gg * gg;
    w -= clr * (gg / (sqrtf(s) + eps));
  }
};

// Adadelta (DL/optim/Adadelta.scala): v = dr·v + (1-dr)·g'² ; upd = sqrt(d+eps)/sqrt(v+eps)·g' ;
// d = dr·d + (1-dr)·upd² ; w -= upd
struct AdadeltaRule {
  static constexpr int NS = 2;
  float scale, dr, omdr, eps;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void step(float& w, float g, float& v, float& d) const {
    const float gg = g * scale;
    v = dr * v + omdr * gg * gg;
    const float upd = sqrtf(d + eps) / sqrtf(v + eps) * gg;
    d = dr * d + omdr * upd * upd;
    w -= upd;
  }
};

// Adamax (DL/optim/Adamax.scala): m = b1·m + (1-b1)·g' ; u = max(b2·u, |g'| + eps) ;
// w -= step·m/u, step = lr / (1 - b1^t) from the host.  An element whose gradient was 0 at every
// step has m = 0 and u = eps (subnormal by default): m/u = 0 exactly, so w keeps its bits.
struct AdamaxRule {
  static constexpr int NS = 2;
  float scale, stepsz, b1, omb1, b2, eps;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void step(float& w, float g, float& m, float& u) const {
    const float gg = g * scale;
    m = b1 * m + omb1 * gg;
    u = fmaxf(b2 * u, fabsf(gg) + eps);
    w -= stepsz * (m / u);
  }
};

// FTRL-proximal in the form of Ftrl._update (the raw gradient squared goes into the accumulator,
// as TensorFlow's FtrlV2): gs = g' + 2·l2s·w ; acc' = acc + g'² ; σ = (acc'^p - acc^p)/lr ;
// lin += gs - σ·w ; quad = acc'^p/lr + 2·l2 ; w = |lin| > l1 ? -(|lin| - l1)·sign(lin)/quad : 0.
// PM selects x^p: 0 = sqrtf (p = 0.5, the default), 1 = the constant 1 (p = 0), 2 = powf.
template <int PM>
struct FtrlRule {
  static constexpr int NS = 2;
  float scale, lr, p, l1, two_l2, two_l2s;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ float pw(float x) const {
    if (PM == 0) return sqrtf(x);
    if (PM == 1) return 1.f;
    return powf(x, p);
  }
  __device__ __forceinline__ void step(float& w, float g, float& acc, float& lin) const {
    const float gg = g * scale;
    const float gs = two_l2s > 0.f ? gg + two_l2s * w : gg;
    const float na = acc + gg * gg;
    const float nap = pw(na);
    const float sigma = (nap - pw(acc)) / lr;
    lin += gs - sigma * w;
    const float quad = nap / lr + two_l2;
    const float al = fabsf(lin);
    const float sgn = lin > 0.f ? 1.f : (lin < 0.f ? -1.f : 0.f);
    w = al > l1 ? -((al - l1) * sgn) / quad : 0.f;
    acc = na;
  }
};

// Adam (DL/optim/Adam.scala): g' = scale·g + wd·w ; m = b1·m + (1-b1)·g' ; v = b2·v + (1-b2)·g'² ;
// w -= step_size·m / (sqrt(v) + eps), step_size = lr·sqrt(1 - b2^t) / (1 - b1^t) from the host, or,
// with dev_n (fp32 [1], the iteration count n before this step, t = n + 1), formed here from the
// decayed rate lr / (1 + n·lr_decay) so that a replayed graph bakes in no host scalar.
struct AdamRule {
  static constexpr int NS = 2;
  float scale, step_size, b1, b2, eps, wd;
  const float* dev_n;
  float lr, lr_decay;
  __device__ __forceinline__ void prepare() {
    if (dev_n) {
      const float n = dev_n[0], t = n + 1.f;
      step_size = lr / (1.f + n * lr_decay) * sqrtf(1.f - powf(b2, t)) / (1.f - powf(b1, t));
    }
  }
  __device__ __forceinline__ void step(float& w, float g, float& m, float& v) const {
    const float gg = g * scale + wd * w;
    m = b1 * m + (1.f - b1) * gg;
    v = b2 * v + (1.f - b2) * gg * gg;
    w -= step_size * m / (sqrtf(v) + eps);
  }
};

// Adagrad (DL/optim/Adagrad.scala): g' = scale·g + wd·w ; s += g'² ; w -= clr·g' / (sqrt(s) + 1e-10),
// clr = lr / (1 + n·lr_decay) from the host, or formed here from dev_n as in AdamRule.
struct AdagradRule {
  static constexpr int NS = 1;
  float scale, clr, wd;
  const float* dev_n;
  float lr, lr_decay;
  __device__ __forceinline__ void prepare() {
    if (dev_n) clr = lr / (1.f + dev_n[0] * lr_decay);
  }
  __device__ __forceinline__ void step(float& w, float g, float& s, float&) const {
    const float gg = g * scale + wd * w;
    s += gg * gg;
    w -= clr * gg / (sqrtf(s) + 1e-10f);
  }
};

// ------------------------------------------------------------------------------------------------
// the kernel: w, s0, s1 16-B aligned, g 16-B (fp32) or 8-B (bf16), shadow 8-B (host-checked);
// s1 is not touched when the rule has one state
// ------------------------------------------------------------------------------------------------
#define K_OPTIM_NAME k_optim
#define K_OPTIM_CLIP 0
#define K_OPTIM_CLIP_PARAMS
#include "k_optim.inc.h"
#undef K_OPTIM_NAME
#undef K_OPTIM_CLIP
#undef K_OPTIM_CLIP_PARAMS
// the same pass with the gradient clipped right after the load (GradClip, optim_common.h)
#define K_OPTIM_NAME k_optim_clip
#define K_OPTIM_CLIP 1
#define K_OPTIM_CLIP_PARAMS , GradClip c, float cscale
#include "k_optim.inc.h"
#undef K_OPTIM_NAME
#undef K_OPTIM_CLIP
#undef K_OPTIM_CLIP_PARAMS

template <typename R, typename G>
static int optim_launch(const R& r, float* w, const G* g, float* s0, float* s1, bf16_t* shadow, long long n,
                        hipStream_t s) {
  if (n <= 0) return 0;
  const long long n4 = n / 4;
  hipLaunchKernelGGL((k_optim<R, G>), dim3(bigdl_grid(n4 > 0 ? n4 : 1, 256)), dim3(256), 0, s, r, w, g, s0, s1,
                     shadow, n4, (int)(n & 3));
  BIGDL_CHECK_LAUNCH();
}

template <typename R, typename G>
static int optim_launch_clip(R r, float* w, const G* g, float* s0, float* s1, bf16_t* shadow, long long n,
                             const GradClip& c, hipStream_t s) {
  if (n <= 0) return 0;
  const long long n4 = n / 4;
  const float scale = r.scale;
  r.scale = 1.f;
  hipLaunchKernelGGL((k_optim_clip<R, G>), dim3(bigdl_grid(n4 > 0 ? n4 : 1, 256)), dim3(256), 0, s, r, w, g, s0, s1,
                     shadow, n4, (int)(n & 3), c, scale);
  BIGDL_CHECK_LAUNCH();
}

// a clipped launch of either gradient type: the _clip entry points take (g, g16) like the LARS ones
template <typename R>
static int optim_clip(const R& r, float* w, const void* g, int g16, float* s0, float* s1, bf16_t* shadow,
                      long long n, const GradClip& c, hipStream_t s) {
  if (g16) return optim_launch_clip(r, w, (const bf16_t*)g, s0, s1, shadow, n, c, s);
  return optim_launch_clip(r, w, (const float*)g, s0, s1, shadow, n, c, s);
}

template <typename G>
static int ftrl_launch(float* w, const G* g, float* acc, float* lin, bf16_t* shadow, long long n, float lr, float p,
                       float l1, float two_l2, float two_l2s, float scale, hipStream_t s) {
  if (p == 0.5f) return optim_launch(FtrlRule<0>{scale, lr, p, l1, two_l2, two_l2s}, w, g, acc, lin, shadow, n, s);
  if (p == 0.f) return optim_launch(FtrlRule<1>{scale, lr, p, l1, two_l2, two_l2s}, w, g, acc, lin, shadow, n, s);
  return optim_launch(FtrlRule<2>{scale, lr, p, l1, two_l2, two_l2s}, w, g, acc, lin, shadow, n, s);
}

// ------------------------------------------------------------------------------------------------
// entry points: n elements; the _g16 twins take a bf16 gradient
// ------------------------------------------------------------------------------------------------
BIGDL_EXPORT int bigdl_rmsprop(float* w, const float* g, float* sq, bf16_t* shadow, long long n, float clr, float dr,
                               float omdr, float eps, float scale, hipStream_t s) {
  return optim_launch(RmspropRule{scale, clr, dr, omdr, eps}, w, g, sq, (float*)nullptr, shadow, n, s);
}

BIGDL_EXPORT int bigdl_rmsprop_g16(float* w, const bf16_t* g, float* sq, bf16_t* shadow, long long n, float clr,
                                   float dr, float omdr, float eps, float scale, hipStream_t s) {
  return optim_launch(RmspropRule{scale, clr, dr, omdr, eps}, w, g, sq, (float*)nullptr, shadow, n, s);
}

BIGDL_EXPORT int bigdl_adadelta(float* w, const float* g, float* v, float* d, bf16_t* shadow, long long n, float dr,
                                float omdr, float eps, float scale, hipStream_t s) {
  return optim_launch(AdadeltaRule{scale, dr, omdr, eps}, w, g, v, d, shadow, n, s);
}

BIGDL_EXPORT int bigdl_adadelta_g16(float* w, const bf16_t* g, float* v, float* d, bf16_t* shadow, long long n,
                                    float dr, float omdr, float eps, float scale, hipStream_t s) {
  return optim_launch(AdadeltaRule{scale, dr, omdr, eps}, w, g, v, d, shadow, n, s);
}

// step = lr / (1 - b1^t)
BIGDL_EXPORT int bigdl_adamax(float* w, const float* g, float* m, float* u, bf16_t* shadow, long long n, float step,
                              float b1, float omb1, float b2, float eps, float scale, hipStream_t s) {
  return optim_launch(AdamaxRule{scale, step, b1, omb1, b2, eps}, w, g, m, u, shadow, n, s);
}

BIGDL_EXPORT int bigdl_adamax_g16(float* w, const bf16_t* g, float* m, float* u, bf16_t* shadow, long long n,
                                  float step, float b1, float omb1, float b2, float eps, float scale, hipStream_t s) {
  return optim_launch(AdamaxRule{scale, step, b1, omb1, b2, eps}, w, g, m, u, shadow, n, s);
}

// p = -learningRatePower; two_l2 = 2·l2, two_l2s = 2·l2Shrinkage
BIGDL_EXPORT int bigdl_ftrl(float* w, const float* g, float* acc, float* lin, bf16_t* shadow, long long n, float lr,
                            float p, float l1, float two_l2, float two_l2s, float scale, hipStream_t s) {
  return ftrl_launch(w, g, acc, lin, shadow, n, lr, p, l1, two_l2, two_l2s, scale, s);
}

BIGDL_EXPORT int bigdl_ftrl_g16(float* w, const bf16_t* g, float* acc, float* lin, bf16_t* shadow, long long n,
                                float lr, float p, float l1, float two_l2, float two_l2s, float scale, hipStream_t s) {
  return ftrl_launch(w, g, acc, lin, shadow, n, lr, p, l1, two_l2, two_l2s, scale, s);
}

// step_size = lr · sqrt(1 - b2^t) / (1 - b1^t)
BIGDL_EXPORT int bigdl_adam(float* w, const float* g, float* m, float* v, bf16_t* shadow, long long n,
                            float step_size, float b1, float b2, float eps, float wd, float scale, hipStream_t s) {
  return optim_launch(AdamRule{scale, step_size, b1, b2, eps, wd, nullptr, 0.f, 0.f}, w, g, m, v, shadow, n, s);
}

BIGDL_EXPORT int bigdl_adam_g16(float* w, const bf16_t* g, float* m, float* v, bf16_t* shadow, long long n,
                                float step_size, float b1, float b2, float eps, float wd, float scale, hipStream_t s) {
  return optim_launch(AdamRule{scale, step_size, b1, b2, eps, wd, nullptr, 0.f, 0.f}, w, g, m, v, shadow, n, s);
}

// dev_n: fp32 [1] iteration count before this step (the caller advances it after the launch)
BIGDL_EXPORT int bigdl_adam_dev(float* w, const float* g, float* m, float* v, bf16_t* shadow, long long n,
                                const float* dev_n, float lr, float lr_decay, float b1, float b2, float eps, float wd,
                                float scale, hipStream_t s) {
  return optim_launch(AdamRule{scale, 0.f, b1, b2, eps, wd, dev_n, lr, lr_decay}, w, g, m, v, shadow, n, s);
}

// dev_n nullable: with it the rate is formed on the device and clr is ignored
BIGDL_EXPORT int bigdl_adagrad(float* w, const float* g, float* sv, bf16_t* shadow, long long n, float clr,
                               const float* dev_n, float lr, float lr_decay, float wd, float scale, hipStream_t s) {
  return optim_launch(AdagradRule{scale, clr, wd, dev_n, lr, lr_decay}, w, g, sv, (float*)nullptr, shadow, n, s);
}

BIGDL_EXPORT int bigdl_adagrad_g16(float* w, const bf16_t* g, float* sv, bf16_t* shadow, long long n, float clr,
                                   const float* dev_n, float lr, float lr_decay, float wd, float scale, hipStream_t s) {
  return optim_launch(AdagradRule{scale, clr, wd, dev_n, lr, lr_decay}, w, g, sv, (float*)nullptr, shadow, n, s);
}

// ------------------------------------------------------------------------------------------------
// clipped entry points: the same updates with a GradClip operand (optim_common.h); g is fp32, or
// bf16 when g16 is set.  sumsq null = no L2 clip; lo / hi = -inf / +inf = no clamp.
// ------------------------------------------------------------------------------------------------
BIGDL_EXPORT int bigdl_rmsprop_clip(float* w, const void* g, int g16, float* sq, bf16_t* shadow, long long n,
                                    float clr, float dr, float omdr, float eps, float scale, const float* sumsq,
                                    float threshold, float lo, float hi, hipStream_t s) {
  return optim_clip(RmspropRule{scale, clr, dr, omdr, eps}, w, g, g16, sq, (float*)nullptr, shadow, n,
                    GradClip{sumsq, threshold, lo, hi}, s);
}

BIGDL_EXPORT int bigdl_adadelta_clip(float* w, const void* g, int g16, float* v, float* d, bf16_t* shadow, long long n,
                                     float dr, float omdr, float eps, float scale, const float* sumsq,
                                     float threshold, float lo, float hi, hipStream_t s) {
  return optim_clip(AdadeltaRule{scale, dr, omdr, eps}, w, g, g16, v, d, shadow, n, GradClip{sumsq, threshold, lo, hi},
                    s);
}

BIGDL_EXPORT int bigdl_adamax_clip(float* w, const void* g, int g16, float* m, float* u, bf16_t* shadow, long long n,
                                   float step, float b1, float omb1, float b2, float eps, float scale,
                                   const float* sumsq, float threshold, float lo, float hi, hipStream_t s) {
  return optim_clip(AdamaxRule{scale, step, b1, omb1, b2, eps}, w, g, g16, m, u, shadow, n,
                    GradClip{sumsq, threshold, lo, hi}, s);
}

BIGDL_EXPORT int bigdl_ftrl_clip(float* w, const void* g, int g16, float* acc, float* lin, bf16_t* shadow, long long n,
                                 float lr, float p, float l1, float two_l2, float two_l2s, float scale,
                                 const float* sumsq, float threshold, float lo, float hi, hipStream_t s) {
  const GradClip c{sumsq, threshold, lo, hi};
  if (p == 0.5f) return optim_clip(FtrlRule<0>{scale, lr, p, l1, two_l2, two_l2s}, w, g, g16, acc, lin, shadow, n, c, s);
  if (p == 0.f) return optim_clip(FtrlRule<1>{scale, lr, p, l1, two_l2, two_l2s}, w, g, g16, acc, lin, shadow, n, c, s);
  return optim_clip(FtrlRule<2>{scale, lr, p, l1, two_l2, two_l2s}, w, g, g16, acc, lin, shadow, n, c, s);
}

// dev_n nullable: with it the step size is formed on the device (bigdl_adam_dev) and step_size is ignored
BIGDL_EXPORT int bigdl_adam_clip(float* w, const void* g, int g16, float* m, float* v, bf16_t* shadow, long long n,
                                 float step_size, const float* dev_n, float lr, float lr_decay, float b1, float b2,
                                 float eps, float wd, float scale, const float* sumsq, float threshold, float lo,
                                 float hi, hipStream_t s) {
  return optim_clip(AdamRule{scale, step_size, b1, b2, eps, wd, dev_n, lr, lr_decay}, w, g, g16, m, v, shadow, n,
                    GradClip{sumsq, threshold, lo, hi}, s);
}

BIGDL_EXPORT int bigdl_adagrad_clip(float* w, const void* g, int g16, float* sv, bf16_t* shadow, long long n, float clr,
                                    const float* dev_n, float lr, float lr_decay, float wd, float scale,
                                    const float* sumsq, float threshold, float lo, float hi, hipStream_t s) {
  return optim_clip(AdagradRule{scale, clr, wd, dev_n, lr, lr_decay}, w, g, g16, sv, (float*)nullptr, shadow, n,
                    GradClip{sumsq, threshold, lo, hi}, s);
}
