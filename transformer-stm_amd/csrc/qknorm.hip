// qknorm.hip — QK-norm: LayerNorm over the head dimension (dh = 64) of the q and k blocks of the
// attention operand qkv [M][ld >= 3*H*64] (q | k | v column blocks, head h at h*64), one gamma / beta
// pair for q and one for k shared by all heads (timm's qk_norm=True with norm_layer=LayerNorm).
//
// HBM-bound streaming kernels.  A row is 3*H*LPH "slots" of 16 bytes (LPH = 8 lanes per head for
// bf16, 16 for fp32), and the grid is a whole number of rows wide (G * 256 threads = R * S slots), so
// thread g keeps slot g % S for the whole launch and walks rows g / S, + R, + 2R, ...: every lane of
// every wave is busy whatever H is, consecutive lanes read consecutive 16 bytes, and the backward's
// column sums stay in registers.  Row sums are xor shuffles inside the head's LPH lanes (LPH divides
// S and 64, so a head never straddles a row, a wave or the end of the loop).
// The backward leaves dbias as one partial row per walked row set (R x 3D, no reduction in the
// kernel: each thread owns its columns) and dgamma / dbeta as one [64] partial per block, summed
// over the block's heads through LDS in a fixed order; fold_rows finishes them (+=, fixed order,
// queued with the LayerNorm folds).  No floating-point atomics.
#include "common.h"
#include <type_traits>

namespace vitmi {

constexpr int QK_DH = 64;
constexpr int QK_BLOCKS = 1024;   // grid cap: 4 blocks of 256 threads per CU

template <typename V>
__device__ __forceinline__ V ldg_s(const V* p) {
  return __builtin_nontemporal_load(p);
}
template <typename V>
__device__ __forceinline__ void put(V* p, V v) {
  __builtin_nontemporal_store(v, p);
}

// 16 bytes of T as floats, and back (one round-to-nearest conversion per element)
template <typename T>
__device__ __forceinline__ void unpack(u32x4 raw, float (&x)[16 / sizeof(T)]) {
  if constexpr (std::is_same_v<T, bf16>) {
    const bf16x8 b = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)b[e];
  } else {
    const f32x4 f = __builtin_bit_cast(f32x4, raw);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = f[e];
  }
}
template <typename T>
__device__ __forceinline__ u32x4 pack(const float (&x)[16 / sizeof(T)]) {
  if constexpr (std::is_same_v<T, bf16>) {
    bf16x8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (bf16)x[e];
    return __builtin_bit_cast(u32x4, b);
  } else {
    return __builtin_bit_cast(u32x4, f32x4{x[0], x[1], x[2], x[3]});
  }
}

template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int o = 1; o < LPH; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- forward
// S = 3*H*LPH slots per row, R = gridDim.x * 256 / S rows per pass.  The v slots copy their 16 bytes.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_fwd_kernel(int64_t M, int H, int S, int64_t R,
                                                         const T* __restrict__ qkv, int64_t ld,
                                                         const float* __restrict__ gamma_q,
                                                         const float* __restrict__ beta_q,
                                                         const float* __restrict__ gamma_k,
                                                         const float* __restrict__ beta_k, float eps,
                                                         T* __restrict__ out, int64_t ldo, float* __restrict__ mean,
                                                         float* __restrict__ rstd) {
  constexpr int EPL = 16 / sizeof(T), LPH = QK_DH / EPL;
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int slot = g % S, hb = slot / LPH, j = slot % LPH;
  const bool isv = hb >= 2 * H;
  const int64_t c = (int64_t)slot * EPL;
  float ga[EPL], be[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    ga[e] = isv ? 0.f : (hb < H ? gamma_q : gamma_k)[j * EPL + e];
    be[e] = isv ? 0.f : (hb < H ? beta_q : beta_k)[j * EPL + e];
  }
  for (int64_t row = g / S; row < M; row += R) {
    const u32x4 raw = ldg_s((const u32x4*)(qkv + row * ld + c));
    float x[EPL];
    unpack<T>(raw, x);
    float s = x[0];
#pragma unroll
    for (int e = 1; e < EPL; ++e) s += x[e];
    const float mu = head_sum<LPH>(s) / QK_DH;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) q += (x[e] - mu) * (x[e] - mu);
    const float rs = rsqrtf(head_sum<LPH>(q) / QK_DH + eps);
    u32x4 o = raw;
    if (!isv) {
      float y[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) y[e] = (x[e] - mu) * rs * ga[e] + be[e];
      o = pack<T>(y);
      if (j == 0) {
        mean[row * (2 * H) + hb] = mu;
        rstd[row * (2 * H) + hb] = rs;
      }
    }
    put((u32x4*)(out + row * ldo + c), o);
  }
}

// ---------------------------------------------------------------- backward
// dqkv's q and k slots in place; part_b [R][3*H*64] (row g / S, the thread's columns; NULL: no dbias,
// and the v slots are not read); part_g [4][gridDim.x][64]: dgamma_q, dbeta_q, dgamma_k, dbeta_k.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_bwd_kernel(int64_t M, int H, int S, int64_t R,
                                                         const T* __restrict__ qkv, int64_t ld,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma_q,
                                                         const float* __restrict__ gamma_k, T* dqkv, int64_t ldd,
                                                         float* __restrict__ part_b, float* __restrict__ part_g) {
  constexpr int EPL = 16 / sizeof(T), LPH = QK_DH / EPL;
  __shared__ float red[2][256][EPL];
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int slot = g % S, hb = slot / LPH, j = slot % LPH;
  const bool isv = hb >= 2 * H;
  const int64_t c = (int64_t)slot * EPL;
  float ga[EPL], dg[EPL], db[EPL], ds[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    ga[e] = isv ? 0.f : (hb < H ? gamma_q : gamma_k)[j * EPL + e];
    dg[e] = db[e] = ds[e] = 0.f;
  }
  for (int64_t row = g / S; row < M; row += R) {
    float x[EPL], dy[EPL];
    float mu = 0.f, rs = 0.f;
    T* dp = dqkv + row * ldd + c;
    if (isv) {
      // the v columns as given, read only for their sums
      if (part_b) {
        unpack<T>(ldg_s((const u32x4*)dp), dy);
#pragma unroll
        for (int e = 0; e < EPL; ++e) ds[e] += dy[e];
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) x[e] = dy[e] = 0.f;
    } else {
      unpack<T>(ldg_s((const u32x4*)(qkv + row * ld + c)), x);
      unpack<T>(ldg_s((const u32x4*)dp), dy);
      mu = mean[row * (2 * H) + hb];
      rs = rstd[row * (2 * H) + hb];
    }
    float xh[EPL], gy[EPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      xh[e] = (x[e] - mu) * rs;
      gy[e] = dy[e] * ga[e];
      s1 += gy[e];
      s2 += gy[e] * xh[e];
    }
    const float c1 = head_sum<LPH>(s1) / QK_DH, c2 = head_sum<LPH>(s2) / QK_DH;
    if (!isv) {
      float o[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        dg[e] += dy[e] * xh[e];
        db[e] += dy[e];
        // dbias sums what is stored: the value rounded to T
        o[e] = to_f32(from_f32<T>((gy[e] - c1 - xh[e] * c2) * rs));
        ds[e] += o[e];
      }
      put((u32x4*)dp, pack<T>(o));
    }
  }
  if (part_b) {
    float* pb = part_b + (int64_t)(g / S) * (3 * H * QK_DH) + c;
#pragma unroll
    for (int e = 0; e < EPL; e += 4) *(f32x4*)(pb + e) = f32x4{ds[e], ds[e + 1], ds[e + 2], ds[e + 3]};
  }
  // dgamma / dbeta of the block: threads t = j, j + LPH, ... hold lane j of some head each; the q heads'
  // and the k heads' are summed in thread order
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    red[0][threadIdx.x][e] = dg[e];
    red[1][threadIdx.x][e] = db[e];
  }
  __syncthreads();
  if (threadIdx.x < 2 * QK_DH) {
    const int which = threadIdx.x / QK_DH, cc = threadIdx.x % QK_DH;   // which: 0 = q, 1 = k
    const int jj = cc / EPL, e = cc % EPL;
    float ag = 0.f, ab = 0.f;
    for (int t = jj; t < 256; t += LPH) {
      const int h2 = ((blockIdx.x * 256 + t) % S) / LPH;
      if (which == 0 ? h2 < H : (h2 >= H && h2 < 2 * H)) {
        ag += red[0][t][e];
        ab += red[1][t][e];
      }
    }
    part_g[((int64_t)(2 * which) * gridDim.x + blockIdx.x) * QK_DH + cc] = ag;
    part_g[((int64_t)(2 * which + 1) * gridDim.x + blockIdx.x) * QK_DH + cc] = ab;
  }
}

// The launch geometry of (M, H, dtype): S slots per row, G blocks (a multiple of the fewest blocks
// that hold whole rows, enough for M rows, at most QK_BLOCKS unless one such multiple is larger),
// R = G * 256 / S rows per pass.
struct QkGeom {
  int S, G;
  int64_t R;
};
static int gcd_(int a, int b) { return b ? gcd_(b, a % b) : a; }
static QkGeom qk_geom(int64_t M, int H, bool bf) {
  const int S = 3 * H * (bf ? 8 : 16);
  const int unit = S / gcd_(S, 256);
  const int64_t need = (M * S + 255) / 256;
  int64_t k = (need + unit - 1) / unit;
  const int64_t kmax = QK_BLOCKS / unit < 1 ? 1 : QK_BLOCKS / unit;
  k = k < 1 ? 1 : k > kmax ? kmax : k;
  const int G = (int)(unit * k);
  return QkGeom{S, G, (int64_t)G * 256 / S};
}
static size_t qk_ws_floats(int64_t M, int H, bool bf) {
  const QkGeom q = qk_geom(M, H, bf);
  return (size_t)q.R * 3 * H * QK_DH + (size_t)4 * q.G * QK_DH;
}

static int qk_check_shape(const char* who, int dtype, int64_t M, int H, int dh, int64_t lda, int64_t ldb) {
  VITMI_CHECK_ARG(dtype == VITMI_F32 || dtype == VITMI_BF16, "%s: dtype must be VITMI_F32 or VITMI_BF16", who);
  VITMI_CHECK_ARG(dh == QK_DH, "%s: dh must be 64 (got %d)", who, dh);
  VITMI_CHECK_ARG(H >= 1 && H <= 32, "%s: H must be in [1, 32] (got %d)", who, H);
  VITMI_CHECK_ARG(M >= 0, "%s: M must not be negative", who);
  const int64_t w = 3LL * H * dh, mult = dtype == VITMI_BF16 ? 8 : 4;
  VITMI_CHECK_ARG(lda >= w && ldb >= w && lda % mult == 0 && ldb % mult == 0,
                  "%s: row strides must be >= 3*H*dh = %lld and multiples of %lld", who, (long long)w, (long long)mult);
  return VITMI_OK;
}

}  // namespace vitmi

using namespace vitmi;

extern "C" int vitmi_qknorm_fwd(int dtype, int64_t M, int H, int dh, const void* qkv, int64_t ld,
                                const float* gamma_q, const float* beta_q, const float* gamma_k,
                                const float* beta_k, float eps, void* out, int64_t ldo, float* mean, float* rstd,
                                vitmi_stream_t stream) {
  if (int rc = qk_check_shape("qknorm_fwd", dtype, M, H, dh, ld, ldo)) return rc;
  if (M == 0) return VITMI_OK;
  VITMI_CHECK_ARG(qkv && gamma_q && beta_q && gamma_k && beta_k && out && mean && rstd, "qknorm_fwd: null pointer");
  VITMI_CHECK_ARG(aligned_to(qkv, 16) && aligned_to(out, 16) && aligned_to(gamma_q, 16) && aligned_to(beta_q, 16) &&
                      aligned_to(gamma_k, 16) && aligned_to(beta_k, 16) && aligned_to(mean, 4) && aligned_to(rstd, 4),
                  "qknorm_fwd: qkv, out, gamma and beta must be 16-byte aligned");
  VITMI_CHECK_ARG(out != qkv, "qknorm_fwd: out must not alias qkv (the backward reads the pre-norm values)");
  const bool bf = dtype == VITMI_BF16;
  const QkGeom q = qk_geom(M, H, bf);
  // qkv read and out written once, the statistics written
  const double bytes = (double)M * 3 * H * dh * (bf ? 2 : 4) * 2 + 16.0 * M * H;
  launch(bf ? untyped(qknorm_fwd_kernel<bf16>) : untyped(qknorm_fwd_kernel<float>), dim3(q.G), dim3(256),
         (hipStream_t)stream, 0, bytes, M, H, q.S, q.R, qkv, ld, gamma_q, beta_q, gamma_k, beta_k, eps, out, ldo, mean,
         rstd);
  VITMI_LAUNCH_CHECK("qknorm_fwd");
  return VITMI_OK;
}

extern "C" size_t vitmi_qknorm_bwd_workspace_size(int64_t M, int H) {
  if (M < 0 || H < 1 || H > 32) return 0;
  const size_t a = qk_ws_floats(M, H, true), b = qk_ws_floats(M, H, false);
  return (a > b ? a : b) * sizeof(float);
}

extern "C" int vitmi_qknorm_bwd(int dtype, int64_t M, int H, int dh, const void* qkv, int64_t ld, const float* mean,
                                const float* rstd, const float* gamma_q, const float* gamma_k, void* dqkv,
                                int64_t ldd, float* dgamma_q, float* dbeta_q, float* dgamma_k, float* dbeta_k,
                                float* dbias, void* workspace, size_t ws_bytes, vitmi_stream_t stream) {
  if (int rc = qk_check_shape("qknorm_bwd", dtype, M, H, dh, ld, ldd)) return rc;
  if (M == 0) return VITMI_OK;
  VITMI_CHECK_ARG(qkv && mean && rstd && gamma_q && gamma_k && dqkv, "qknorm_bwd: null pointer");
  VITMI_CHECK_ARG(aligned_to(qkv, 16) && aligned_to(dqkv, 16) && aligned_to(gamma_q, 16) && aligned_to(gamma_k, 16) &&
                      aligned_to(workspace, 16) && aligned_to(mean, 4) && aligned_to(rstd, 4) &&
                      aligned_to(dgamma_q, 4) && aligned_to(dbeta_q, 4) && aligned_to(dgamma_k, 4) &&
                      aligned_to(dbeta_k, 4) && aligned_to(dbias, 4),
                  "qknorm_bwd: qkv, dqkv, gamma and the workspace must be 16-byte aligned");
  VITMI_CHECK_ARG(dqkv != qkv, "qknorm_bwd: dqkv must not alias qkv");
  VITMI_CHECK_ARG(workspace && ws_bytes >= vitmi_qknorm_bwd_workspace_size(M, H), "qknorm_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const bool bf = dtype == VITMI_BF16;
  const QkGeom q = qk_geom(M, H, bf);
  const int64_t W = 3LL * H * dh;
  float* part_b = dbias ? (float*)workspace : nullptr;
  float* part_g = (float*)workspace + q.R * W;
  // q and k: qkv and dqkv read, dqkv written; v read for dbias; the statistics read; the partials written
  const double bytes = (double)M * H * dh * (bf ? 2 : 4) * (6 + (dbias ? 1 : 0)) + 16.0 * M * H +
                       4.0 * ((dbias ? (double)q.R * W : 0.0) + 4.0 * q.G * dh);
  launch(bf ? untyped(qknorm_bwd_kernel<bf16>) : untyped(qknorm_bwd_kernel<float>), dim3(q.G), dim3(256), s, 0, bytes,
         M, H, q.S, q.R, qkv, ld, mean, rstd, gamma_q, gamma_k, dqkv, ldd, part_b, part_g);
  VITMI_LAUNCH_CHECK("qknorm_bwd");
  float* const outs[4] = {dgamma_q, dbeta_q, dgamma_k, dbeta_k};
  for (int i = 0; i < 4; ++i)
    if (int rc = fold_rows(part_g + (int64_t)i * q.G * dh, q.G, dh, dh, outs[i], s)) return rc;
  return fold_rows(part_b, q.R, W, W, dbias, s);
}
