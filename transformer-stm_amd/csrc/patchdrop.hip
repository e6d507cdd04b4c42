// patchdrop.hip — patch dropout (timm's patch_drop_rate, FLIP, the MAE encoder's random masking):
// each sample keeps the K of its np patches with the smallest (key, p) pairs, key(b, p) =
// vitmi_dropout_hash(seed, site, b, p) (include/vitmi.h, "Patch dropout").  The selection kernel
// writes the kept patch numbers in ascending order (keep) and their inverse (slot); the gathered
// im2col, token assembly and position-gradient kernels read those.  An index outside [0, np) is
// "no patch": the forward kernels write a zero row, the backward adds nothing.
#include "common.h"

namespace vitmi {

constexpr int KEEP_MAX_NP = 4096;
constexpr int KEEP_THREADS = 256;

// ------------------------------------------------------------ selection
// One block per sample.  The keys sit in LDS (padded to a multiple of 4 with 0xFFFFFFFF at
// positions >= np, which no (key, p) pair of a real patch is larger than); a thread ranks each of
// its patches by counting the smaller pairs, four keys per 16-byte LDS read (every lane reads the
// same address: a broadcast).  The ranks are a permutation of 0..np-1, so exactly K patches have
// rank < K.  Patches are handled in chunks of blockDim in ascending order; a ballot prefix count
// inside each chunk plus the running total of the chunks before it is the patch's position j in
// the ascending keep list.
__global__ __launch_bounds__(KEEP_THREADS) void patch_keep_kernel(int np, int K, uint32_t seed, uint32_t site,
                                                                  int* __restrict__ keep, int* __restrict__ slot) {
  __shared__ u32x4 keys4[KEEP_MAX_NP / 4];
  __shared__ int wcnt[KEEP_THREADS / 64];
  uint32_t* keys = (uint32_t*)keys4;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t rk = drop_row_key(seed, site, (uint32_t)b);
  const int np4 = (np + 3) / 4;
  for (int p = tid; p < np4 * 4; p += KEEP_THREADS) keys[p] = p < np ? drop_hash(rk, (uint32_t)p) : 0xFFFFFFFFu;
  __syncthreads();
  int* keep_b = keep + (int64_t)b * K;
  int* slot_b = slot + (int64_t)b * np;
  int base = 0;
  for (int p0 = 0; p0 < np; p0 += KEEP_THREADS) {   // block-uniform trip count
    const int p = p0 + tid;
    bool kept = false;
    if (p < np) {
      const uint32_t k = keys[p];
      int rank = 0;
      for (int q4 = 0; q4 < np4; ++q4) {
        const u32x4 kq = keys4[q4];
#pragma unroll
        for (int e = 0; e < 4; ++e) rank += (kq[e] < k) || (kq[e] == k && q4 * 4 + e < p);
      }
      kept = rank < K;
    }
    const uint64_t m = __ballot(kept);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < KEEP_THREADS / 64; ++w) {
      const int c = wcnt[w];
      if (w < wave) off += c;
      total += c;
    }
    if (p < np) {
      const int j = kept ? off + __popcll(m & ((1ull << lane) - 1ull)) : -1;
      slot_b[p] = j;
      if (kept) keep_b[j] = p;   // j < K: the kept patches number exactly K
    }
    base += total;
    __syncthreads();             // wcnt is rewritten by the next chunk
  }
}

// ------------------------------------------------------------ gathered im2col
// im2col_kernel (elementwise.hip) with row b*K + j reading patch keep[b][j]: one block per
// output row, one thread per 4 consecutive kw.  Kc = C*P*P.
template <typename T>
__global__ __launch_bounds__(1024) void im2col_keep_kernel(const float* __restrict__ img, T* __restrict__ out, int C,
                                                           int S, int P, int K, const int* __restrict__ keep) {
  const int G = S / P, np = G * G, Kc = C * P * P;
  const int row = blockIdx.x;                        // b * K + j
  const int b = row / K;
  const int pidx = keep[row];
  const int col = threadIdx.x * 4;
  if (col >= Kc) return;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (pidx >= 0 && pidx < np) {
    const int ph = pidx / G, pw = pidx - ph * G;
    const int c = col / (P * P), r = col - c * P * P, kh = r / P, kw = r - kh * P;
    v = *(const f32x4*)(img + (((int64_t)b * C + c) * S + ph * P + kh) * S + pw * P + kw);
  }
  T* o = out + (int64_t)row * Kc + col;
  if constexpr (sizeof(T) == 2) {
    bf16x4 w;
    w[0] = (bf16)v[0]; w[1] = (bf16)v[1]; w[2] = (bf16)v[2]; w[3] = (bf16)v[3];
    *(bf16x4*)o = w;
  } else {
    *(f32x4*)o = v;
  }
}

// ------------------------------------------------------------ gathered token assembly
// x[b][0] = cls + pos[0];  x[b][1+j] = tok[b*K+j] + pos[1 + keep[b][j]]
__global__ void tokens_assemble_keep_kernel(int B, int np, int K, int D, const float* __restrict__ tok,
                                            const float* __restrict__ cls, const float* __restrict__ pos,
                                            const int* __restrict__ keep, float* __restrict__ x) {
  const int N = K + 1, D4 = D / 4;
  const int64_t total = (int64_t)B * N * D4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4) * 4;
    const int64_t bn = i / D4;
    const int n = (int)(bn % N);
    const int64_t b = bn / N;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n == 0) {
      if (cls) v = *(const f32x4*)(cls + d);
      if (pos) v += *(const f32x4*)(pos + d);
    } else {
      const int64_t r = b * K + n - 1;
      const int pidx = keep[r];
      if (pidx >= 0 && pidx < np) {
        v = *(const f32x4*)(tok + r * D + d);
        if (pos) v += *(const f32x4*)(pos + (int64_t)(1 + pidx) * D + d);
      }
    }
    *(f32x4*)(x + bn * D + d) = v;
  }
}

// ------------------------------------------------------------ position / cls gradient
// dpos[0][d] += sum_b dx[b][0][d] (and dcls[d] +=);  dpos[1+p][d] += sum over the samples that
// kept p of dx[b][1 + slot[b][p]][d].  One thread per (n, d), b ascending, no atomics: the sum is
// bitwise reproducible.  8 slots, then 8 rows, in flight per thread (tokens_pos_bwd_kernel).
__global__ void tokens_pos_keep_bwd_kernel(int B, int np, int K, int D, const float* __restrict__ dx,
                                           const int* __restrict__ slot, float* __restrict__ dcls,
                                           float* __restrict__ dpos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)(np + 1) * D) return;
  const int n = (int)(i / D), d = (int)(i % D);
  const int64_t st = (int64_t)(K + 1) * D;          // one sample of dx
  const float* base = dx + d;
  const bool tok0 = n == 0;                         // the cls row: every sample, row 0
  const int* sl = slot + (tok0 ? 0 : n - 1);
  float s = 0.f;
  int b = 0;
  for (; b + 8 <= B; b += 8) {
    int r[8];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = tok0 ? -1 : sl[(int64_t)(b + j) * np];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = tok0 || (r[j] >= 0 && r[j] < K) ? base[(b + j) * st + (int64_t)(r[j] + 1) * D] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; b < B; ++b) {
    const int r = tok0 ? -1 : sl[(int64_t)b * np];
    if (tok0 || (r >= 0 && r < K)) s += base[b * st + (int64_t)(r + 1) * D];
  }
  if (dpos) dpos[i] += s;
  if (dcls && n == 0) dcls[d] += s;
}

}  // namespace vitmi

using namespace vitmi;

#define PATCHDROP_CHECK_GEOM(what)                                                                      \
  VITMI_CHECK_ARG(B > 0 && K >= 1 && K <= np && np <= KEEP_MAX_NP, what ": need B > 0 and 1 <= K <= np <= 4096")

extern "C" int vitmi_patch_keep(int B, int np, int K, uint32_t seed, uint32_t site, int32_t* keep, int32_t* slot,
                                vitmi_stream_t stream) {
  PATCHDROP_CHECK_GEOM("patch_keep");
  VITMI_CHECK_ARG(keep && slot, "patch_keep: null pointer");
  launch(patch_keep_kernel, dim3((unsigned)B), dim3(KEEP_THREADS), (hipStream_t)stream, no_stat, np, K, seed, site,
         keep, slot);
  VITMI_LAUNCH_CHECK("patch_keep");
  return VITMI_OK;
}

extern "C" int vitmi_patch_im2col_keep(int dtype, int B, int C, int S, int P, int K, const int32_t* keep,
                                       const float* img, void* patches, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(P > 0 && S > 0 && C > 0 && S % P == 0 && P % 4 == 0,
                  "im2col_keep: need S %% P == 0 and P %% 4 == 0");
  const int64_t np = (int64_t)(S / P) * (S / P);
  PATCHDROP_CHECK_GEOM("im2col_keep");
  VITMI_CHECK_ARG(keep && img && patches, "im2col_keep: null pointer");
  VITMI_CHECK_ARG(dtype == VITMI_BF16 || dtype == VITMI_F32, "im2col_keep: bad dtype");
  const int64_t Kc = (int64_t)C * P * P, rows = (int64_t)B * K;
  VITMI_CHECK_ARG(Kc / 4 <= 1024 && rows < 0x7fffffff, "im2col_keep: C*P*P must be <= 4096");
  const dim3 block((unsigned)((Kc / 4 + 63) / 64 * 64));
  launch(dtype == VITMI_BF16 ? untyped(im2col_keep_kernel<bf16>) : untyped(im2col_keep_kernel<float>),
         dim3((unsigned)rows), block, (hipStream_t)stream, no_stat, img, patches, C, S, P, K, keep);
  VITMI_LAUNCH_CHECK("im2col_keep");
  return VITMI_OK;
}

extern "C" int vitmi_tokens_assemble_keep(int B, int np, int K, int D, const float* tok, const float* cls,
                                          const float* pos, const int32_t* keep, float* x, vitmi_stream_t stream) {
  PATCHDROP_CHECK_GEOM("tokens_assemble_keep");
  VITMI_CHECK_ARG(D > 0 && D % 4 == 0, "tokens_assemble_keep: D %% 4 != 0");
  VITMI_CHECK_ARG(tok && keep && x, "tokens_assemble_keep: null pointer");
  const int64_t work = (int64_t)B * (K + 1) * D / 4;
  launch(tokens_assemble_keep_kernel, dim3(grid_cap(work)), dim3(256), (hipStream_t)stream, no_stat, B, np, K, D, tok,
         cls, pos, keep, x);
  VITMI_LAUNCH_CHECK("tokens_assemble_keep");
  return VITMI_OK;
}

extern "C" int vitmi_tokens_assemble_keep_bwd(int B, int np, int K, int D, const float* dx, float* dtok,
                                              void* dtok_lp, float* dcls, float* dpos, const int32_t* slot,
                                              vitmi_stream_t stream) {
  PATCHDROP_CHECK_GEOM("tokens_assemble_keep_bwd");
  VITMI_CHECK_ARG(D > 0 && D % 4 == 0, "tokens_assemble_keep_bwd: D %% 4 != 0");
  VITMI_CHECK_ARG(dx && slot, "tokens_assemble_keep_bwd: null pointer");
  // the kept rows of a sample are contiguous in dx: the split is the full one at np = K
  if (dtok || dtok_lp)
    if (int rc = vitmi_tokens_assemble_bwd(B, K, D, dx, dtok, dtok_lp, nullptr, nullptr, stream)) return rc;
  if (dcls || dpos) {
    const int64_t work = (int64_t)(np + 1) * D;
    launch(tokens_pos_keep_bwd_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), (hipStream_t)stream, no_stat, B,
           np, K, D, dx, slot, dcls, dpos);
  }
  VITMI_LAUNCH_CHECK("tokens_assemble_keep_bwd");
  return VITMI_OK;
}
