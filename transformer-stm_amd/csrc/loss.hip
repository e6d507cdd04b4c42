// loss.hip — the classification recipe on the device, gfx950: softmax cross-entropy with label,
// mixed-pair (mixup / cutmix) and dense soft targets, label smoothing and top-1 / top-k scoring in
// one pass over the logits, and the mixup / cutmix image pass.
//
// vitmi_softmax_xent: one wave64 per logits row.  Pass 1 reads the row once (16-byte loads when
// every row base is aligned and C % 4 == 0, scalar loads otherwise), keeps it in registers when
// C <= XENT_REG_ELEMS, and forms per lane a running (max, sum exp) pair, the row sum of z (label
// smoothing), the dense target's sums, and the count of classes ranked in front of the label.  The
// lanes are combined with the wave's xor butterfly (every lane ends with the same bits; no LDS, no
// atomics).  Pass 2 writes the gradient from the registers, or re-reads the row (L2) when it did
// not fit.  A row's results depend on that row and C alone: not on B, the grid or the block size.
// The finalize launch (one block) folds the per-row losses in fp64 in a fixed order, as
// vitmi_clip_finalize folds its partials, and adds the batch to the metrics record.
//
// vitmi_mix_batch: out = box ? img[perm] : lam img + (1 - lam) img[perm], explicitly rounded fp32
// products and one addition (the file is built with -ffp-contract=off), bit-identical to a float32
// NumPy evaluation.  One block per 4096-element chunk of one [H][W] plane, so the per-sample
// tables are read once per block and a thread does one division (row of its group) per 16 bytes.
#include "common.h"

#include <math.h>

namespace vitmi {
namespace {

// ---------------------------------------------------------------- softmax cross-entropy
constexpr int XENT_REG_ELEMS = 1024;   // 16 floats per lane: ImageNet-1k rows stay in registers
constexpr int XENT_REG = XENT_REG_ELEMS / 64;

struct XentArgs {
  int B, C;
  const float* z;
  int64_t ldl;
  const int64_t* la;
  const int64_t* lb;
  const float* lam;
  const float* soft;
  int64_t lds;
  float smoothing;
  int topk;
  float* row_loss;   // the caller's, or the workspace's: never null when the finalize launch runs
  float* dl;
  int64_t lddl;
  uint8_t* flags;    // per row: bit 0 top-1 hit, bit 1 top-k hit (null without metrics)
  float invB;
};

// The 32-byte metrics record of include/vitmi.h.
struct ClassRec {
  double loss_sum;
  uint64_t rows, top1, topk;
};
static_assert(sizeof(ClassRec) == 32, "the metrics record is 32 bytes (include/vitmi.h)");

template <int W>
__device__ __forceinline__ void ld_w(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const f32x4 t = *(const f32x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = t[j];
  } else {
    v[0] = p[0];
  }
}
template <int W>
__device__ __forceinline__ void st_w(float* p, const float (&v)[W]) {
  if constexpr (W == 4) {
    *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    p[0] = v[0];
  }
}

__device__ __forceinline__ int wave_sum_i(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// what one lane carries through pass 1
struct XentAcc {
  float m, s;       // running max and sum of exp(z - m) of this lane's elements
  float sz;         // sum of z (the smoothing term)
  float st, stz;    // dense targets: sum of t, sum of t z over t != 0
  int cnt;          // classes ranked in front of the label
};

template <int W, bool DENSE>
__device__ __forceinline__ void xent_take(XentAcc& a, const float (&v)[W], const float* trow, int c, float zy, int y) {
  float vm = v[0];
#pragma unroll
  for (int j = 1; j < W; ++j) vm = fmaxf(vm, v[j]);
  if (vm > a.m) {          // exp(-inf - vm) = 0 and s is 0 then: the first finite element starts the sum
    a.s *= expf(a.m - vm);
    a.m = vm;
  }
  if (a.m != -INFINITY) {
#pragma unroll
    for (int j = 0; j < W; ++j) a.s += expf(v[j] - a.m);
  } else {                 // every element so far is -inf or NaN: -inf adds nothing (and forms no inf - inf),
#pragma unroll             // a NaN (which no max rises for) goes into the sum and stays through every rescale
    for (int j = 0; j < W; ++j)
      if (v[j] != v[j]) a.s = v[j];
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    a.sz += v[j];
    a.cnt += (v[j] > zy || (v[j] == zy && c + j < y)) ? 1 : 0;
  }
  if constexpr (DENSE) {
    float t[W];
    ld_w<W>(trow + c, t);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      a.st += t[j];
      if (t[j] != 0.f) a.stz += t[j] * v[j];   // a zero-weight class adds nothing, even at z = -inf
    }
  }
}

// blockDim.x / 64 rows per block, one wave each; no block-level synchronisation
template <int W, bool DENSE>
__global__ __launch_bounds__(256) void softmax_xent_kernel(XentArgs p) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= p.B) return;
  const int C = p.C;
  const float* zrow = p.z + (int64_t)b * p.ldl;
  const float* trow = DENSE ? p.soft + (int64_t)b * p.lds : nullptr;

  // the label scored (and, in the label form, weighted): outside [0, C) it matches no class
  const int64_t la64 = p.la ? p.la[b] : -1;
  const int ia = (la64 >= 0 && la64 < C) ? (int)la64 : -1;
  const float za = ia >= 0 ? zrow[ia] : __builtin_nanf("");   // NaN: every comparison below is false

  XentAcc a{-INFINITY, 0.f, 0.f, 0.f, 0.f, 0};
  float r[XENT_REG];
  constexpr int NR = XENT_REG / W;        // register-resident steps of W elements
  // every load of the register part is issued before the first exp waits for one
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int c = (lane + 64 * i) * W;
    float v[W];
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = -INFINITY;
    if (c < C) ld_w<W>(zrow + c, v);      // W == 4 only with C % 4 == 0: a group is whole or absent
#pragma unroll
    for (int j = 0; j < W; ++j) r[i * W + j] = v[j];
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int c = (lane + 64 * i) * W;
    if (c < C) {
      float v[W];
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = r[i * W + j];
      xent_take<W, DENSE>(a, v, trow, c, za, ia);
    }
  }
  for (int c = (lane + 64 * NR) * W; c < C; c += 64 * W) {
    float v[W];
    ld_w<W>(zrow + c, v);
    xent_take<W, DENSE>(a, v, trow, c, za, ia);
  }

  // combine the lanes
  const float M = wave_max(a.m);
  // a lane that met no finite element holds s = 0, or the NaN it met
  const float se = wave_sum(a.m == -INFINITY ? a.s : a.s * expf(a.m - M));
  const float lse = M + logf(se);
  const int cnt = wave_sum_i(a.cnt);

  // target weights: S = sum(t); the uniform part of q is smoothing * S / C
  float wa = 0.f, wb = 0.f, S, dot;
  int ib = -1;
  if constexpr (DENSE) {
    S = wave_sum(a.st);
    dot = wave_sum(a.stz);
  } else {
    wa = 1.f;
    if (p.lam) {
      wa = p.lam[b];
      wb = 1.f - wa;
      const int64_t lb64 = p.lb[b];
      ib = (lb64 >= 0 && lb64 < C) ? (int)lb64 : -1;
    }
    S = p.lam ? wa + wb : 1.f;
    dot = 0.f;
    if (ia >= 0 && wa != 0.f) dot += wa * za;
    if (ib >= 0 && wb != 0.f) dot += wb * zrow[ib];
  }
  const float keep = 1.f - p.smoothing;
  const float unif = p.smoothing > 0.f ? p.smoothing * S / (float)C : 0.f;
  // sum(q) = S; sum(q z) from the indexed logits (or the dense sums) plus the row sum of z.  Without
  // smoothing the row sum stays out: it is -inf for a row with masked classes
  const float sumz = p.smoothing > 0.f ? wave_sum(a.sz) : 0.f;
  if (p.row_loss && lane == 0) {
    float qz = keep * dot;
    if (p.smoothing > 0.f) qz += unif * sumz;
    p.row_loss[b] = lse * S - qz;
  }
  if (p.flags && lane == 0) {
    const bool scored = ia >= 0 && za == za;                // a NaN at the label is a miss
    p.flags[b] = (uint8_t)((scored && cnt < 1 ? 1 : 0) | (scored && cnt < p.topk ? 2 : 0));
  }
  if (!p.dl) return;

  // gradient: (softmax(z) S - q) / B, softmax as exp(z - max) / sum
  const float inv = 1.f / se;
  float* drow = p.dl + (int64_t)b * p.lddl;
  auto grad = [&](const float (&v)[W], int c) {
    float t[W], g[W];
    if constexpr (DENSE) {
      ld_w<W>(trow + c, t);
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) t[j] = (c + j == ia ? wa : 0.f) + (c + j == ib ? wb : 0.f);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float q = p.smoothing > 0.f ? keep * t[j] + unif : t[j];
      g[j] = (expf(v[j] - M) * inv * S - q) * p.invB;
    }
    st_w<W>(drow + c, g);
  };
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int c = (lane + 64 * i) * W;
    if (c < C) {
      float v[W];
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = r[i * W + j];
      grad(v, c);
    }
  }
  for (int c = (lane + 64 * NR) * W; c < C; c += 64 * W) {
    float v[W];
    ld_w<W>(zrow + c, v);
    grad(v, c);
  }
}

__device__ __forceinline__ double xent_wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// One block of 256: thread t adds rows t, t + 256, ... in ascending order (fp64), wave butterfly,
// then ((w0 + w1) + w2) + w3 through LDS.  The hit counts are integers: any order gives the same.
__global__ __launch_bounds__(256) void xent_finalize_kernel(int B, const float* __restrict__ row_loss,
                                                           const uint8_t* __restrict__ flags,
                                                           float* __restrict__ loss, ClassRec* __restrict__ rec) {
  __shared__ double sh[4];
  __shared__ int sh1[4], shk[4];
  double acc = 0.0;
  int h1 = 0, hk = 0;
  for (int i = threadIdx.x; i < B; i += 256) {
    acc += (double)row_loss[i];
    if (flags) {
      const int f = flags[i];
      h1 += f & 1;
      hk += (f >> 1) & 1;
    }
  }
  acc = xent_wave_sum_f64(acc);
  h1 = wave_sum_i(h1);
  hk = wave_sum_i(hk);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = acc;
    sh1[threadIdx.x >> 6] = h1;
    shk[threadIdx.x >> 6] = hk;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double total = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  if (loss) loss[0] = (float)(total / (double)B);
  if (rec) {
    rec->loss_sum = rec->loss_sum + total;
    rec->rows = rec->rows + (uint64_t)B;
    rec->top1 = rec->top1 + (uint64_t)(sh1[0] + sh1[1] + sh1[2] + sh1[3]);
    rec->topk = rec->topk + (uint64_t)(shk[0] + shk[1] + shk[2] + shk[3]);
  }
}

// ---------------------------------------------------------------- mixup / cutmix
constexpr int MIX_THREADS = 256;
constexpr int MIX_U = 4;   // groups per thread: four 16-B loads per operand in flight

struct MixArgs {
  int B, C, H, W;
  const float* img;
  float* out;
  const int* perm;
  const float* lam;
  const int* box;
  uint32_t chunks;   // blocks per [H][W] plane
};

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <int W4>   // elements per group: 4 (16-byte path, W % 4 == 0) or 1
__global__ __launch_bounds__(MIX_THREADS) void mix_batch_kernel(MixArgs p) {
  const uint32_t plane = blockIdx.x / p.chunks;            // b * C + c
  const uint32_t chunk = blockIdx.x - plane * p.chunks;
  const int b = (int)(plane / (uint32_t)p.C);
  int pb = p.perm[b];
  if (pb < 0 || pb >= p.B) pb = b;
  const float lam = p.lam[b];
  const float oml = __fsub_rn(1.f, lam);
  const int y0 = clampi(p.box[4 * b + 0], 0, p.H), y1 = clampi(p.box[4 * b + 1], 0, p.H);
  const int x0 = clampi(p.box[4 * b + 2], 0, p.W), x1 = clampi(p.box[4 * b + 3], 0, p.W);
  const bool empty = y0 >= y1 || x0 >= x1;
  const bool copy = empty && lam == 1.f;                   // the partner is not read
  const int64_t hw = (int64_t)p.H * p.W;
  const float* a = p.img + (int64_t)plane * hw;
  const float* q = p.img + ((int64_t)pb * p.C + (plane - (uint32_t)b * p.C)) * hw;
  float* o = p.out + (int64_t)plane * hw;
  const uint32_t gw = (uint32_t)p.W / W4;                   // groups per image row
  const uint32_t groups = (uint32_t)p.H * gw;
  const uint32_t g0 = chunk * (MIX_THREADS * MIX_U) + threadIdx.x;
  float av[MIX_U][W4], qv[MIX_U][W4];
#pragma unroll
  for (int u = 0; u < MIX_U; ++u) {
    const uint32_t g = g0 + u * MIX_THREADS;
    if (g < groups) {
      ld_w<W4>(a + (int64_t)g * W4, av[u]);
      if (!copy) ld_w<W4>(q + (int64_t)g * W4, qv[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < MIX_U; ++u) {
    const uint32_t g = g0 + u * MIX_THREADS;
    if (g >= groups) break;
    float r[W4];
    if (copy) {
#pragma unroll
      for (int j = 0; j < W4; ++j) r[j] = av[u][j];
    } else {
      const int y = (int)(g / gw);
      const int x = (int)(g - (uint32_t)y * gw) * W4;
      const bool yin = !empty && y >= y0 && y < y1;
#pragma unroll
      for (int j = 0; j < W4; ++j) {
        const bool in = yin && x + j >= x0 && x + j < x1;
        r[j] = in ? qv[u][j] : __fadd_rn(__fmul_rn(lam, av[u][j]), __fmul_rn(oml, qv[u][j]));
      }
    }
    if constexpr (W4 == 4) __builtin_nontemporal_store(f32x4{r[0], r[1], r[2], r[3]}, (f32x4*)(o + (int64_t)g * 4));
    else o[g] = r[0];
  }
}

}  // namespace
}  // namespace vitmi

using namespace vitmi;

extern "C" size_t vitmi_softmax_xent_workspace_size(int B) {
  // fp32 row losses (when the caller keeps none) + one flag byte per row, each part 16-byte rounded
  return B <= 0 ? 0 : (((size_t)B * 4 + 15) / 16 * 16) + (((size_t)B + 15) / 16 * 16);
}

extern "C" int vitmi_softmax_xent(int B, int C, const float* logits, int64_t ldl, const int64_t* label_a,
                                  const int64_t* label_b, const float* lam, const float* soft, int64_t lds,
                                  float smoothing, int topk, float* row_loss, float* loss, float* dlogits,
                                  int64_t lddl, void* metrics, void* workspace, size_t workspace_bytes,
                                  vitmi_stream_t stream) {
  VITMI_CHECK_ARG(B > 0, "softmax_xent: B must be > 0 (got %d)", B);
  VITMI_CHECK_ARG(C >= 1 && C <= 65535, "softmax_xent: C must be in 1..65535 (got %d)", C);
  VITMI_CHECK_ARG(logits != nullptr, "softmax_xent: null logits");
  VITMI_CHECK_ARG(ldl >= C, "softmax_xent: ldl %lld < C %d", (long long)ldl, C);
  VITMI_CHECK_ARG(smoothing >= 0.f && smoothing < 1.f, "softmax_xent: smoothing must be in [0, 1) (got %g)",
                  (double)smoothing);
  VITMI_CHECK_ARG(topk >= 0 && topk <= C, "softmax_xent: topk must be in 0..C (got %d, C %d)", topk, C);
  VITMI_CHECK_ARG(row_loss || loss || dlogits || metrics, "softmax_xent: every output is null");
  VITMI_CHECK_ARG(soft || label_a, "softmax_xent: label_a is required without a dense target");
  VITMI_CHECK_ARG((label_b != nullptr) == (lam != nullptr), "softmax_xent: label_b and lam go together");
  VITMI_CHECK_ARG(!soft || !label_b, "softmax_xent: a dense target takes no label_b / lam pair");
  VITMI_CHECK_ARG(!soft || lds >= C, "softmax_xent: lds %lld < C %d", (long long)lds, C);
  VITMI_CHECK_ARG(!dlogits || lddl >= C, "softmax_xent: lddl %lld < C %d", (long long)lddl, C);
  if (metrics) {
    VITMI_CHECK_ARG(label_a != nullptr, "softmax_xent: metrics are scored against label_a, which is null");
    VITMI_CHECK_ARG(topk >= 1, "softmax_xent: topk must be >= 1 with metrics");
    VITMI_CHECK_ARG(aligned_to(metrics, 16), "softmax_xent: the metrics record must be 16-byte aligned");
  }
  const bool finalize = loss || metrics;
  const bool need_ws = metrics || (loss && !row_loss);
  if (need_ws) {
    VITMI_CHECK_ARG(workspace != nullptr && workspace_bytes >= vitmi_softmax_xent_workspace_size(B),
                    "softmax_xent: workspace too small (%zu < %zu bytes)", workspace ? workspace_bytes : (size_t)0,
                    vitmi_softmax_xent_workspace_size(B));
    VITMI_CHECK_ARG(aligned_to(workspace, 4), "softmax_xent: the workspace must be 4-byte aligned");
  }
  float* rows = row_loss ? row_loss : (finalize ? (float*)workspace : nullptr);
  uint8_t* flags = metrics ? (uint8_t*)workspace + ((size_t)B * 4 + 15) / 16 * 16 : nullptr;

  XentArgs a{B, C, logits, ldl, label_a, label_b, lam, soft, lds, smoothing, topk, rows, dlogits, lddl, flags,
             1.f / (float)B};
  // 16-byte row accesses need every row base of every array the kernel touches aligned
  const bool vec = C % 4 == 0 && aligned_to(logits, 16) && ldl % 4 == 0 && aligned_to(soft, 16) &&
                   (!soft || lds % 4 == 0) && aligned_to(dlogits, 16) && (!dlogits || lddl % 4 == 0);
  // one row per wave; small batches take one wave per block so the rows spread over the CUs
  const int rpb = B >= 2048 ? 4 : 1;
  const dim3 grid((unsigned)((B + rpb - 1) / rpb)), block(64 * rpb);
  void (*kern)(XentArgs) = vec ? (soft ? softmax_xent_kernel<4, true> : softmax_xent_kernel<4, false>)
                               : (soft ? softmax_xent_kernel<1, true> : softmax_xent_kernel<1, false>);
  // the logits once (a row past the registers a second time, from L2), the dense target, the gradient
  const double n = (double)B * C;
  launch(kern, grid, block, (hipStream_t)stream, 0, n * 4 * (1 + (soft ? 1 : 0) + (dlogits ? 1 : 0)) + (double)B * 16,
         a);
  VITMI_LAUNCH_CHECK("softmax_xent");
  if (finalize) {
    launch(xent_finalize_kernel, dim3(1), dim3(256), (hipStream_t)stream, 0, (double)B * 5 + (metrics ? 64.0 : 0.0) + 4,
           B, (const float*)rows, (const uint8_t*)flags, loss, (ClassRec*)metrics);
    VITMI_LAUNCH_CHECK("softmax_xent finalize");
  }
  return VITMI_OK;
}

extern "C" int vitmi_mix_batch(int B, int C, int H, int W, const float* img, const int* perm, const float* lam,
                               const int* box, float* out, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "mix_batch: dimensions must be positive (got %d %d %d %d)", B, C,
                  H, W);
  VITMI_CHECK_ARG(img && perm && lam && box && out, "mix_batch: null pointer");
  const int64_t hw = (int64_t)H * W;
  VITMI_CHECK_ARG(hw <= 0x7fffffff && (int64_t)B * C <= 0x7fffffff, "mix_batch: plane or plane count too large");
  const int64_t n = (int64_t)B * C * hw;
  VITMI_CHECK_ARG(out + n <= img || img + n <= out, "mix_batch: out must not alias img");
  const bool vec = W % 4 == 0 && aligned_to(img, 16) && aligned_to(out, 16);
  const int64_t groups = vec ? hw / 4 : hw;
  const int64_t chunks = (groups + MIX_THREADS * MIX_U - 1) / (MIX_THREADS * MIX_U);
  const int64_t blocks = chunks * B * C;
  VITMI_CHECK_ARG(blocks <= 0x7fffffff, "mix_batch: batch too large for one launch");
  MixArgs a{B, C, H, W, img, out, perm, lam, box, (uint32_t)chunks};
  void (*kern)(MixArgs) = vec ? mix_batch_kernel<4> : mix_batch_kernel<1>;
  // the batch read as itself and as the partner, written once; the three tables
  launch(kern, dim3((unsigned)blocks), dim3(MIX_THREADS), (hipStream_t)stream, 0, (double)n * 12 + (double)B * 24, a);
  VITMI_LAUNCH_CHECK("mix_batch");
  return VITMI_OK;
}
