// optim.hip — the reference's optimizer step, fused, gfx950.
//
// model.compile(optimizer=keras.optimizers.Adam(learning_rate=1e-3)) (models/CvT(Par).py:458-460)
// with Keras' Adam update (beta_1 0.9, beta_2 0.999, epsilon 1e-7; the "epsilon hat" form: eps
// is added to sqrt(v) WITHOUT bias correction, the bias corrections are folded into the step):
//
//   m <- m + (g - m)(1 - b1);   v <- v + (g^2 - v)(1 - b2)
//   p <- p - alpha m / (sqrt(v) + eps),   alpha = lr sqrt(1 - b2^t) / (1 - b1^t)  (host, fp32)
//
// One launch over a ParamArena's flat fp32 buffers (all parameters, gradients, m, v at the same
// offsets); optionally writes the bf16 operand shadow of the updated parameters in the same pass
// (what the next forward's GEMMs read), so no separate cast pass is needed.  HBM-bound:
// 16 B read + 12 B written per parameter (+2 B with the shadow).  Every operation is an
// explicitly rounded IEEE fp32 op in the order above (no FMA contraction), so the result is
// bit-identical to a numpy float32 evaluation of the same formula (oracle/optim_ref.py).
#include "common.h"

namespace vitmi {

struct AdamArgs {
  float alpha, one_m_b1, one_m_b2, eps, grad_scale;
};

__device__ __forceinline__ void adam1(const AdamArgs& a, float& p, float g, float& m, float& v) {
  // HIP's __f*_rn are plain operators (and __fsqrt_rn is the native approximation): the file is
  // built with -ffp-contract=off (Makefile) so a*b+c stays two roundings; sqrtf and / are
  // correctly rounded in HIP by default
  if (a.grad_scale != 1.f) g = __fmul_rn(g, a.grad_scale);
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), a.one_m_b1));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), a.one_m_b2));
  const float den = __fadd_rn(sqrtf(v), a.eps);
  p = __fsub_rn(p, __fdiv_rn(__fmul_rn(m, a.alpha), den));
}

// streaming (non-temporal) loads and stores
template <typename V>
__device__ __forceinline__ V ld_s(const V* q) {
  return __builtin_nontemporal_load(q);
}
template <typename V>
__device__ __forceinline__ void st_s(V* q, V x) {
  __builtin_nontemporal_store(x, q);
}

// ---------------------------------------------------------------- global-norm clipping
// The device record the clipped / skippable step reads (vitmi_clip_finalize writes it).
struct ClipCtl {
  float coef;              // what the step multiplies the (scaled) gradients by; exactly 1 = no clipping
  float norm;              // |grad_scale| * sqrt(sum g^2)
  uint32_t skip;           // 1: this step leaves p, m, v as they are
  uint32_t skipped_total;  // running count of skipped steps
};
static_assert(sizeof(ClipCtl) == 16, "the clip record is 16 bytes (include/vitmi.h)");

// Sum of squares of one chunk per block, in fp64, in a fixed order (bitwise reproducible, and
// independent of the grid: a chunk's partial depends on its SUMSQ_CHUNK elements alone):
//   thread t holds the 16-B groups t, t + 256, ..., t + 256 (U - 1) of the chunk; element e of
//   its groups goes to accumulator a[e], groups in ascending order; thread sum (a0 + a1) + (a2 + a3);
//   wave sum: xor butterfly 32, 16, ..., 1 (every lane ends with the same bits); block sum
//   ((w0 + w1) + w2) + w3 through LDS.
// (double)g squared is exact (48 significant bits), so only the additions round.  Elements past n
// count as +0, which leaves every partial's bits unchanged (all terms are >= +0).
// Measured at the ViT-B arena (85.8 M elements, 343 MB; tools/optim_bench.py): 50-51 us alone, and
// 58 us more per step with the finalize launch.  Chunk 2048 / 4096 / 8192 / 16384 / 32768 elements:
// 49 / 50 / 51 / 52 / 52 us (same process, alternating); the finalize block's serial fold grows
// with the partial count, so 8192.
constexpr int SUMSQ_THREADS = 256;
constexpr int SUMSQ_U = VITMI_GRAD_SUMSQ_CHUNK / (SUMSQ_THREADS * 4);
static_assert(SUMSQ_U >= 1 && SUMSQ_U * SUMSQ_THREADS * 4 == VITMI_GRAD_SUMSQ_CHUNK &&
                  (VITMI_GRAD_SUMSQ_CHUNK & (VITMI_GRAD_SUMSQ_CHUNK - 1)) == 0,
              "the chunk is a power of two and a whole number of 16-B groups per thread");

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// block sum of 256 threads' values in the fixed order above; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double x, double* sh) {
  x = wave_sum_f64(x);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_kernel(int64_t n, const float* __restrict__ g,
                                                                  double* __restrict__ partials) {
  __shared__ double sh[SUMSQ_THREADS / 64];
  const int64_t n4 = n / 4;
  const int64_t base4 = (int64_t)blockIdx.x * (VITMI_GRAD_SUMSQ_CHUNK / 4) + threadIdx.x;
  f32x4 x[SUMSQ_U];
#pragma unroll
  for (int u = 0; u < SUMSQ_U; ++u) {
    const int64_t i = base4 + (int64_t)u * SUMSQ_THREADS;
    if (i < n4) {
      x[u] = ld_s((const f32x4*)g + i);
    } else {
      x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i == n4) {   // the n % 4 tail sits in the group after the last whole one
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (i * 4 + e < n) x[u][e] = g[i * 4 + e];
      }
    }
  }
  double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < SUMSQ_U; ++u) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)x[u][e];
      a[e] += d * d;
    }
  }
  const double s = block_sum_f64((a[0] + a[1]) + (a[2] + a[3]), sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One block: thread t adds partials t, t + 256, ... in ascending order, then the block sum above.
__global__ __launch_bounds__(SUMSQ_THREADS) void clip_finalize_kernel(int64_t n_partials,
                                                                     const double* __restrict__ partials,
                                                                     float grad_scale, float clip_norm,
                                                                     int skip_nonfinite, ClipCtl* __restrict__ ctl) {
  __shared__ double sh[SUMSQ_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_partials; i += SUMSQ_THREADS) acc += partials[i];
  const double total = block_sum_f64(acc, sh);
  if (threadIdx.x != 0) return;
  const bool finite = isfinite(total);
  const float norm = (float)(fabs((double)grad_scale) * sqrt(total));
  float coef = 1.f;
  if (!finite) coef = __builtin_nanf("");          // nothing hidden: the step's results become NaN
  else if (clip_norm > 0.f && norm > clip_norm) coef = __fdiv_rn(clip_norm, norm);
  const uint32_t skip = (skip_nonfinite && !finite) ? 1u : 0u;
  ctl->coef = coef;
  ctl->norm = norm;
  ctl->skip = skip;
  ctl->skipped_total = ctl->skipped_total + skip;
}

// adam1 with the clip coefficient and the decoupled weight decay in front (the step of
// vitmi_adam_step_ctl); with coef == 1 and decay == false it is adam1's ops exactly
__device__ __forceinline__ void adam1_ctl(const AdamArgs& a, float coef, bool decay, float wd, float lr, float& p,
                                          float g, float& m, float& v) {
  if (a.grad_scale != 1.f) g = __fmul_rn(g, a.grad_scale);
  if (coef != 1.f) g = __fmul_rn(g, coef);
  if (decay) p = __fsub_rn(p, __fmul_rn(__fmul_rn(p, wd), lr));
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), a.one_m_b1));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), a.one_m_b2));
  const float den = __fadd_rn(sqrtf(v), a.eps);
  p = __fsub_rn(p, __fdiv_rn(__fmul_rn(m, a.alpha), den));
}

// what a skipped step still does: lp = bf16(p) over the thread's groups (and its tail element)
__device__ __forceinline__ void shadow_only(int64_t n4, int64_t first, int64_t stride, bool tail, int64_t t,
                                            const float* __restrict__ p, bf16* __restrict__ lp) {
  for (int64_t i = first; i < n4; i += stride) {
    const f32x4 pv = ld_s((const f32x4*)p + i);
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = from_f32<bf16>(pv[e]);
    ((bf16x4*)lp)[i] = o;
  }
  if (tail) lp[t] = from_f32<bf16>(p[t]);
}

// ---------------------------------------------------------------- EMA of the weights
// keras.optimizers.Adam(use_ema=True): e <- mom e + (1 - mom) p_new, three rounded fp32 ops on the
// parameter the step has just produced (one_m = 1 - mom is formed on the host, in fp32).
__device__ __forceinline__ float ema1(float e, float p, float mom, float one_m) {
  return __fadd_rn(__fmul_rn(mom, e), __fmul_rn(one_m, p));
}

// ---------------------------------------------------------------- the step kernel
// One loop behind the three step entry points; the switches are compile-time, so an instance holds
// nothing of the others' lines:
//   <LP, false, false>  vitmi_adam_step: adam1; no trace of coef, decay or the record.
//   <LP, true, false>   vitmi_adam_step_ctl: adam1_ctl, the record read once per thread.  A skipped step
//                       reads p alone and writes only the shadow.  mask: one byte per 64 elements (16
//                       consecutive 16-B groups).
//   <LP, true, true>    vitmi_adam_step_ema: the same with the average as a fifth stream, 4 B read and
//                       4 B written per parameter on top.  A skipped step neither reads nor writes e.
// LP: the bf16 shadow of the new p, a plain 8-B store.  ADAM_U = two 16-B groups per thread in flight,
// every load issued before the first use, non-temporal loads and stores of the fp32 streams; the
// first threads of the grid take n % 4.  Measured at the ViT-B arena, us per step:
//   <true, false, false> (tools/ln_bench.py, same box, A/B): 504-526 as written, 573-595 with plain
//     loads and stores and one group in flight.
//   <true, true, true> (tools/ema_bench.py, two processes of three rounds each): 546-564 as written,
//     580-588 with a plain load of e, 600-604 with one group in flight.
static constexpr int ADAM_U = 2;
template <bool LP, bool CTL, bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16* __restrict__ lp, AdamArgs a, float wd, float lr,
                                                   const uint8_t* __restrict__ mask, const ClipCtl* __restrict__ ctl,
                                                   float* __restrict__ ema, float mom, float one_m) {
  static_assert(CTL || !EMA, "the average rides on the ctl step");
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t t = n4 * 4 + first;   // tail (n % 4) by the first threads
  const bool tail = t < n && t < n4 * 4 + 4;
  float coef = 1.f;
  if constexpr (CTL) {
    coef = ctl ? ctl->coef : 1.f;
    if (ctl && ctl->skip) {
      if constexpr (LP) shadow_only(n4, first, stride, tail, t, p, lp);
      return;
    }
  }
  constexpr int U = ADAM_U;
  for (int64_t i0 = first; i0 < n4; i0 += U * stride) {
    f32x4 pv[U], gv[U], mv[U], vv[U], ev[U];
    bool dec[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if constexpr (CTL) dec[u] = false;
      if (u == 0 || i < n4) {
        pv[u] = ld_s((const f32x4*)p + i);
        gv[u] = ld_s((const f32x4*)g + i);
        mv[u] = ld_s((const f32x4*)m + i);
        vv[u] = ld_s((const f32x4*)v + i);
        if constexpr (EMA) ev[u] = ld_s((const f32x4*)ema + i);
        if constexpr (CTL) dec[u] = wd != 0.f && (!mask || mask[i >> 4] != 0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (u > 0 && i >= n4) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[u][e], me = mv[u][e], ve = vv[u][e];
        if constexpr (CTL) adam1_ctl(a, coef, dec[u], wd, lr, pe, gv[u][e], me, ve);
        else adam1(a, pe, gv[u][e], me, ve);
        pv[u][e] = pe;
        mv[u][e] = me;
        vv[u][e] = ve;
        if constexpr (EMA) ev[u][e] = ema1(ev[u][e], pe, mom, one_m);
      }
      st_s((f32x4*)p + i, pv[u]);
      st_s((f32x4*)m + i, mv[u]);
      st_s((f32x4*)v + i, vv[u]);
      if constexpr (EMA) st_s((f32x4*)ema + i, ev[u]);
      if constexpr (LP) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<bf16>(pv[u][e]);
        ((bf16x4*)lp)[i] = o;
      }
    }
  }
  if (tail) {
    float pe = p[t], me = m[t], ve = v[t];
    if constexpr (CTL) adam1_ctl(a, coef, wd != 0.f && (!mask || mask[t >> 6] != 0), wd, lr, pe, g[t], me, ve);
    else adam1(a, pe, g[t], me, ve);
    p[t] = pe;
    m[t] = me;
    v[t] = ve;
    if constexpr (EMA) ema[t] = ema1(ema[t], pe, mom, one_m);
    if constexpr (LP) lp[t] = from_f32<bf16>(pe);
  }
}

// Using the average: SWAP exchanges p and ema in place (a thread loads both 16-B groups at its
// index, then stores both: no temporary), otherwise p <- ema; the shadow of the new p rides along.
template <bool LP, bool SWAP>
__global__ __launch_bounds__(256) void ema_apply_kernel(int64_t n, float* __restrict__ p, float* __restrict__ ema,
                                                        bf16* __restrict__ lp) {
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n4; i += stride) {
    const f32x4 ev = ld_s((const f32x4*)ema + i);
    if constexpr (SWAP) {
      const f32x4 pv = ld_s((const f32x4*)p + i);
      st_s((f32x4*)ema + i, pv);
    }
    st_s((f32x4*)p + i, ev);
    if constexpr (LP) {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = from_f32<bf16>(ev[e]);
      ((bf16x4*)lp)[i] = o;
    }
  }
  const int64_t t = n4 * 4 + first;   // tail (n % 4) by the first threads
  if (t < n && t < n4 * 4 + 4) {
    const float ee = ema[t];
    if constexpr (SWAP) ema[t] = p[t];
    p[t] = ee;
    if constexpr (LP) lp[t] = from_f32<bf16>(ee);
  }
}

}  // namespace vitmi

using namespace vitmi;

// What the three step entry points share: every check, the arguments, the recorded bytes and the
// launch.  `what` is the entry point's name; ctl_form / ema_form say which instance it runs, whatever
// the values (vitmi_adam_step passes weight_decay 0 and null decay_mask, ctl and ema).  Value
// arguments are judged before the n == 0 return, pointers after it.
static int adam_launch(const char* what, bool ctl_form, bool ema_form, int64_t n, float* p, const float* g, float* m,
                       float* v, void* p_lp, float alpha, double beta_1, double beta_2, float epsilon,
                       float grad_scale, float weight_decay, float lr, const uint8_t* decay_mask, const void* ctl,
                       float* ema, float ema_momentum, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(n >= 0, "%s: n < 0", what);
  VITMI_CHECK_ARG(beta_1 >= 0.0 && beta_1 < 1.0 && beta_2 >= 0.0 && beta_2 < 1.0 && epsilon >= 0.f,
                  "%s: bad hyper-parameters", what);
  VITMI_CHECK_ARG(weight_decay >= 0.f, "%s: weight_decay must be >= 0", what);
  VITMI_CHECK_ARG(ema_momentum >= 0.f && ema_momentum < 1.f, "%s: ema_momentum must be in [0, 1)", what);
  if (n == 0) return VITMI_OK;
  VITMI_CHECK_ARG(p && g && m && v && (ema || !ema_form), "%s: null pointer", what);
  VITMI_CHECK_ARG(aligned_to(p, 16) && aligned_to(g, 16) && aligned_to(m, 16) && aligned_to(v, 16) &&
                      aligned_to(ema, 16),
                  "%s: fp32 buffers must be 16-byte aligned", what);
  VITMI_CHECK_ARG(aligned_to(p_lp, 8), "%s: bf16 shadow must be 8-byte aligned", what);
  VITMI_CHECK_ARG(aligned_to(ctl, 16), "%s: the clip record must be 16-byte aligned", what);
  // (1 - beta) in double then rounded once, as Keras does with its Python-float hyper-parameters
  AdamArgs a{alpha, (float)(1.0 - beta_1), (float)(1.0 - beta_2), epsilon, grad_scale};
  // p, g, m, v (+ the average) read; p, m, v (+ the average, + the bf16 shadow) written; plus the mask
  // bytes and the record (a skipped step moves less: not known here)
  const double bytes = (double)n * ((ema_form ? 36 : 28) + (p_lp ? 2 : 0)) +
                       (decay_mask && weight_decay != 0.f ? (double)((n + 63) / 64) : 0.0) + (ctl ? 16.0 : 0.0);
  auto kernel = ema_form   ? (p_lp ? adam_kernel<true, true, true> : adam_kernel<false, true, true>)
                : ctl_form ? (p_lp ? adam_kernel<true, true, false> : adam_kernel<false, true, false>)
                           : (p_lp ? adam_kernel<true, false, false> : adam_kernel<false, false, false>);
  launch(kernel, dim3(grid_cap(n / 4)), dim3(256), (hipStream_t)stream, 0, bytes, n, p, g, m, v, (bf16*)p_lp, a,
         weight_decay, lr, decay_mask, (const ClipCtl*)ctl, ema, ema_momentum, 1.f - ema_momentum);
  VITMI_LAUNCH_CHECK(what);
  return VITMI_OK;
}

extern "C" int vitmi_adam_step(int64_t n, float* p, const float* g, float* m, float* v, void* p_lp, float alpha,
                               double beta_1, double beta_2, float epsilon, float grad_scale, vitmi_stream_t stream) {
  return adam_launch("adam_step", false, false, n, p, g, m, v, p_lp, alpha, beta_1, beta_2, epsilon, grad_scale, 0.f,
                     0.f, nullptr, nullptr, nullptr, 0.f, stream);
}

extern "C" size_t vitmi_grad_sumsq_partials(int64_t n) {
  return n <= 0 ? 0 : (size_t)((n + VITMI_GRAD_SUMSQ_CHUNK - 1) / VITMI_GRAD_SUMSQ_CHUNK);
}

extern "C" int vitmi_grad_sumsq(int64_t n, const float* g, double* partials, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(n >= 0, "grad_sumsq: n < 0");
  if (n == 0) return VITMI_OK;
  VITMI_CHECK_ARG(g && partials, "grad_sumsq: null pointer");
  VITMI_CHECK_ARG(aligned_to(g, 16), "grad_sumsq: the gradient buffer must be 16-byte aligned");
  VITMI_CHECK_ARG(aligned_to(partials, 8), "grad_sumsq: partials must be 8-byte aligned");
  const size_t chunks = vitmi_grad_sumsq_partials(n);
  VITMI_CHECK_ARG(chunks <= 0x7fffffffu, "grad_sumsq: n too large for one launch");
  // g read once; one double per chunk written
  launch(grad_sumsq_kernel, dim3((unsigned)chunks), dim3(SUMSQ_THREADS), (hipStream_t)stream, 0,
         (double)n * 4 + (double)chunks * 8, n, g, partials);
  VITMI_LAUNCH_CHECK("grad_sumsq");
  return VITMI_OK;
}

extern "C" int vitmi_clip_finalize(int64_t n_partials, const double* partials, float grad_scale, float clip_norm,
                                   int skip_nonfinite, void* ctl, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(n_partials >= 0, "clip_finalize: n_partials < 0");
  VITMI_CHECK_ARG(ctl && (partials || n_partials == 0), "clip_finalize: null pointer");
  VITMI_CHECK_ARG(aligned_to(partials, 8), "clip_finalize: partials must be 8-byte aligned");
  VITMI_CHECK_ARG(aligned_to(ctl, 16), "clip_finalize: the clip record must be 16-byte aligned");
  VITMI_CHECK_ARG(clip_norm >= 0.f, "clip_finalize: clip_norm must be >= 0 (0 = off)");
  launch(clip_finalize_kernel, dim3(1), dim3(SUMSQ_THREADS), (hipStream_t)stream, 0,
         (double)n_partials * 8 + 2 * sizeof(ClipCtl), n_partials, partials, grad_scale, clip_norm, skip_nonfinite,
         (ClipCtl*)ctl);
  VITMI_LAUNCH_CHECK("clip_finalize");
  return VITMI_OK;
}

extern "C" int vitmi_adam_step_ctl(int64_t n, float* p, const float* g, float* m, float* v, void* p_lp, float alpha,
                                   double beta_1, double beta_2, float epsilon, float grad_scale, float weight_decay,
                                   float lr, const uint8_t* decay_mask, const void* ctl, vitmi_stream_t stream) {
  return adam_launch("adam_step_ctl", true, false, n, p, g, m, v, p_lp, alpha, beta_1, beta_2, epsilon, grad_scale,
                     weight_decay, lr, decay_mask, ctl, nullptr, 0.f, stream);
}

extern "C" int vitmi_adam_step_ema(int64_t n, float* p, const float* g, float* m, float* v, void* p_lp, float alpha,
                                   double beta_1, double beta_2, float epsilon, float grad_scale, float weight_decay,
                                   float lr, const uint8_t* decay_mask, const void* ctl, float* ema,
                                   float ema_momentum, vitmi_stream_t stream) {
  return adam_launch("adam_step_ema", true, true, n, p, g, m, v, p_lp, alpha, beta_1, beta_2, epsilon, grad_scale,
                     weight_decay, lr, decay_mask, ctl, ema, ema_momentum, stream);
}

extern "C" int vitmi_ema_apply(int64_t n, float* p, float* ema, void* p_lp, int mode, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(n >= 0, "ema_apply: n < 0");
  VITMI_CHECK_ARG(mode == 0 || mode == 1, "ema_apply: mode must be 0 (swap) or 1 (copy)");
  if (n == 0) return VITMI_OK;
  VITMI_CHECK_ARG(p && ema, "ema_apply: null pointer");
  VITMI_CHECK_ARG(aligned_to(p, 16) && aligned_to(ema, 16), "ema_apply: fp32 buffers must be 16-byte aligned");
  VITMI_CHECK_ARG(aligned_to(p_lp, 8), "ema_apply: bf16 shadow must be 8-byte aligned");
  const bool swap = mode == 0;
  auto kernel = p_lp ? (swap ? ema_apply_kernel<true, true> : ema_apply_kernel<true, false>)
                     : (swap ? ema_apply_kernel<false, true> : ema_apply_kernel<false, false>);
  // swap: p and ema read and written; copy: ema read, p written (+ the bf16 shadow)
  launch(kernel, dim3(grid_cap(n / 4)), dim3(256), (hipStream_t)stream, 0,
         (double)n * ((swap ? 16 : 8) + (p_lp ? 2 : 0)), n, p, ema, (bf16*)p_lp);
  VITMI_LAUNCH_CHECK("ema_apply");
  return VITMI_OK;
}
