// LayerScale (CaiT; timm init_values=, blocks.i.ls{1,2}.gamma): the learned per-channel scale of a
// residual branch, folded into the weight operand of the branch's last GEMM (include/vitmi.h,
// "LayerScale").  Four memory-bound kernels, 16-byte accesses, no atomics: every sum runs in an
// order fixed by the shape alone, so results are bitwise reproducible.
#include "common.h"

namespace vitmi {

// w_eff[n][k] = round(gamma[n] * w[n][k]) (one fp32 multiply, then RNE to TO); bias_eff[n] = gamma[n]
// * b[n].  One thread per 8 consecutive k of a row (two 16-byte loads; one 16-byte bf16 store or two
// fp32 ones), grid-stride over the N * K / 8 units; the first N threads also write the bias.
template <typename TO>
__global__ __launch_bounds__(256) void layerscale_fold_kernel(uint32_t units, uint32_t k8, int64_t N,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ gamma,
                                                               TO* __restrict__ w_eff, const float* __restrict__ b,
                                                               float* __restrict__ b_eff) {
  const uint32_t t0 = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
  if (b_eff != nullptr)
    for (int64_t n = t0; n < N; n += step) b_eff[n] = gamma[n] * b[n];
  for (uint32_t i = t0; i < units; i += step) {
    const float g = gamma[i / k8];
    const float* p = w + (int64_t)i * 8;
    f32x4 a = *(const f32x4*)p, c = *(const f32x4*)(p + 4);
    a *= g;
    c *= g;
    if constexpr (sizeof(TO) == 4) {
      *(f32x4*)(w_eff + (int64_t)i * 8) = a;
      *(f32x4*)(w_eff + (int64_t)i * 8 + 4) = c;
    } else {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (bf16)a[e];
        o[4 + e] = (bf16)c[e];
      }
      *(bf16x8*)(w_eff + (int64_t)i * 8) = o;
    }
  }
}

// One row n per WPR waves of a 256-thread block (WPR = 1: four rows per block; 4: one).  In one pass
// over the row: acc += dw[n][k] * w[n][k] (DOT) and dw[n][k] *= gamma[n] (SCALE), four k per lane and
// step.  The row's sum: each lane's k in ascending order, the wave's xor butterfly, then the WPR wave
// sums in wave order; dgamma[n] += that + db[n] * b[n]; db[n] *= gamma[n] last.
template <int WPR, bool DOT, bool SCALE>
__global__ __launch_bounds__(256) void layerscale_bwd_kernel(int64_t N, int64_t K, const float* __restrict__ w,
                                                              const float* __restrict__ b,
                                                              const float* __restrict__ gamma, float* __restrict__ dw,
                                                              float* __restrict__ db, float* __restrict__ dgamma) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = WPR == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x;
  const bool live = n < N;                                     // wave-uniform
  float acc = 0.f;
  if (live && dw != nullptr) {
    const float g = SCALE ? gamma[n] : 0.f;
    const int64_t k4 = K / 4;
    float* drow = dw + n * K;
    const float* wrow = w + n * K;
    for (int64_t c = WPR == 1 ? lane : threadIdx.x; c < k4; c += 64 * WPR) {
      f32x4 d = *(const f32x4*)(drow + c * 4);
      if constexpr (DOT) {
        const f32x4 v = *(const f32x4*)(wrow + c * 4);
        acc += d[0] * v[0];
        acc += d[1] * v[1];
        acc += d[2] * v[2];
        acc += d[3] * v[3];
      }
      if constexpr (SCALE) {
        d *= g;
        *(f32x4*)(drow + c * 4) = d;
      }
    }
  }
  if constexpr (DOT) {
    acc = wave_sum(acc);
    if constexpr (WPR == 4) {
      if (lane == 0) red[wave] = acc;
      __syncthreads();
      acc = ((red[0] + red[1]) + red[2]) + red[3];
    }
  }
  const bool first = lane == 0 && (WPR == 1 || wave == 0);
  if (live && first) {
    if constexpr (DOT) dgamma[n] += db != nullptr ? acc + db[n] * b[n] : acc;
    if constexpr (SCALE)
      if (db != nullptr) db[n] *= gamma[n];
  }
}

// y[r][c] = x[r][c] * gamma[c]; four columns per thread (N % 4 == 0)
template <typename TO>
__global__ __launch_bounds__(256) void layerscale_apply_kernel(int64_t M, int64_t N, const float* __restrict__ x,
                                                                int64_t ldx, const float* __restrict__ gamma,
                                                                TO* __restrict__ y, int64_t ldy) {
  const int64_t n4 = N / 4, total = M * n4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / n4, c = (i - r * n4) * 4;
    const f32x4 o = *(const f32x4*)(x + r * ldx + c) * *(const f32x4*)(gamma + c);
    if constexpr (sizeof(TO) == 4) {
      *(f32x4*)(y + r * ldy + c) = o;
    } else {
      bf16x4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = (bf16)o[e];
      *(bf16x4*)(y + r * ldy + c) = h;
    }
  }
}

// part[z][c] = sum over the rows m of chunk z of dy[m][c] * x[m][c].  256 threads = 4 row groups x 64
// lanes of four columns; group g takes rows m0 + g, m0 + g + 4, ... in ascending order, then the four
// group sums are added in group order (the first step of the column reduction; fold_rows is the second).
__global__ __launch_bounds__(256) void layerscale_dgamma_kernel(int64_t M, int64_t N, const float* __restrict__ dy,
                                                                 int64_t lddy, const float* __restrict__ x,
                                                                 int64_t ldx, float* __restrict__ part,
                                                                 int64_t rows_per) {
  __shared__ f32x4 red[4][64];
  const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * 4;
  const int64_t m0 = (int64_t)blockIdx.y * rows_per;
  const int64_t m1 = m0 + rows_per < M ? m0 + rows_per : M;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (c < N) {
#pragma unroll 4
    for (int64_t m = m0 + rg; m < m1; m += 4) a += *(const f32x4*)(dy + m * lddy + c) * *(const f32x4*)(x + m * ldx + c);
  }
  red[rg][lane] = a;
  __syncthreads();
  if (rg == 0 && c < N)
    *(f32x4*)(part + (int64_t)blockIdx.y * N + c) = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// row chunks of the column reduction: about 1024 blocks, at least 32 rows per chunk, at most 256
static int dgamma_splits(int64_t M, int64_t N) {
  const int64_t colblocks = (N + 255) / 256;
  int64_t z = 1024 / (colblocks < 1 ? 1 : colblocks);
  const int64_t zmax = (M + 31) / 32;
  if (z > zmax) z = zmax;
  if (z > 256) z = 256;
  return (int)(z < 1 ? 1 : z);
}

}  // namespace vitmi

using namespace vitmi;

extern "C" int vitmi_layerscale_fold(int64_t N, int64_t K, const float* w, const float* gamma, const float* bias,
                                     void* w_eff, int w_dtype, float* bias_eff, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(w && gamma && w_eff, "layerscale_fold: null pointer (w, gamma and w_eff are required)");
  VITMI_CHECK_ARG((bias == nullptr) == (bias_eff == nullptr),
                  "layerscale_fold: bias and bias_eff are given together or both null");
  VITMI_CHECK_ARG(w_dtype == VITMI_F32 || w_dtype == VITMI_BF16, "layerscale_fold: bad w_dtype %d", w_dtype);
  VITMI_CHECK_ARG(N >= 1, "layerscale_fold: N must be >= 1 (got %lld)", (long long)N);
  VITMI_CHECK_ARG(K >= 8 && K % 8 == 0, "layerscale_fold: K must be a positive multiple of 8 (got %lld)",
                  (long long)K);
  VITMI_CHECK_ARG(N <= (int64_t)0x7fffffff && K <= (int64_t)0x7fffffff && N * (K / 8) <= (int64_t)0x7fffffff,
                  "layerscale_fold: N * K / 8 must be < 2^31");
  VITMI_CHECK_ARG(aligned_to(w, 16) && aligned_to(w_eff, 16), "layerscale_fold: w and w_eff must be 16-byte aligned");
  const uint32_t k8 = (uint32_t)(K / 8), units = (uint32_t)(N * (K / 8));
  const bool f32 = w_dtype == VITMI_F32;
  // 8 blocks per CU at the most: a [768, 3072] weight is 1152 blocks, every unit touched once
  launch(f32 ? untyped(layerscale_fold_kernel<float>) : untyped(layerscale_fold_kernel<bf16>),
         dim3(grid_cap(units, 256, 2048)), dim3(256), (hipStream_t)stream, 0, (f32 ? 8.0 : 6.0) * N * K, units, k8, N,
         w, gamma, w_eff, bias, bias_eff);
  VITMI_LAUNCH_CHECK("layerscale_fold");
  return VITMI_OK;
}

extern "C" int vitmi_layerscale_bwd(int64_t N, int64_t K, const float* w, const float* bias, const float* gamma,
                                    float* dw, float* db, float* dgamma, int scale_grads, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(scale_grads == 0 || scale_grads == 1, "layerscale_bwd: scale_grads must be 0 or 1 (got %d)",
                  scale_grads);
  VITMI_CHECK_ARG(dw || db, "layerscale_bwd: null pointer (dw or db is required)");
  VITMI_CHECK_ARG(!dgamma || (dw && w), "layerscale_bwd: null pointer (dgamma needs dw and w)");
  VITMI_CHECK_ARG(!db || !dgamma || bias, "layerscale_bwd: null pointer (dgamma with db needs bias)");
  VITMI_CHECK_ARG(!scale_grads || gamma, "layerscale_bwd: null pointer (scale_grads needs gamma)");
  VITMI_CHECK_ARG(N >= 1, "layerscale_bwd: N must be >= 1 (got %lld)", (long long)N);
  VITMI_CHECK_ARG(K >= 8 && K % 8 == 0, "layerscale_bwd: K must be a positive multiple of 8 (got %lld)",
                  (long long)K);
  VITMI_CHECK_ARG(N <= (int64_t)0x7fffffff && K <= (int64_t)0x7fffffff, "layerscale_bwd: N and K must be < 2^31");
  VITMI_CHECK_ARG(aligned_to(w, 16) && aligned_to(dw, 16), "layerscale_bwd: w and dw must be 16-byte aligned");
  if (!dgamma && !scale_grads) return VITMI_OK;   // frozen gamma, gradients in temporaries: nothing to do
  const hipStream_t s = (hipStream_t)stream;
  const bool wide = K > 1024;                     // a block per row from 4 KiB rows on, a wave below
  const dim3 grid((unsigned)(wide ? N : (N + 3) / 4));
  const double bytes = (dw ? 4.0 * N * K : 0.0) * ((dgamma ? 2 : 1) + (scale_grads ? 1 : 0));
  // [wide][dgamma and scale_grads, dgamma alone, scale_grads alone]
  static constexpr decltype(&layerscale_bwd_kernel<1, true, true>) kern[2][3] = {
      {layerscale_bwd_kernel<1, true, true>, layerscale_bwd_kernel<1, true, false>,
       layerscale_bwd_kernel<1, false, true>},
      {layerscale_bwd_kernel<4, true, true>, layerscale_bwd_kernel<4, true, false>,
       layerscale_bwd_kernel<4, false, true>}};
  launch(kern[wide][dgamma ? (scale_grads ? 0 : 1) : 2], grid, dim3(256), s, dgamma ? 2.0 * N * K : 0.0, bytes, N, K, w,
         bias, gamma, dw, db, dgamma);
  VITMI_LAUNCH_CHECK("layerscale_bwd");
  return VITMI_OK;
}

extern "C" int vitmi_layerscale_apply(int64_t M, int64_t N, const float* x, int64_t ldx, const float* gamma, void* y,
                                      int y_dtype, int64_t ldy, vitmi_stream_t stream) {
  VITMI_CHECK_ARG(x && gamma && y, "layerscale_apply: null pointer");
  VITMI_CHECK_ARG(y_dtype == VITMI_F32 || y_dtype == VITMI_BF16, "layerscale_apply: bad dtype %d", y_dtype);
  VITMI_CHECK_ARG(M >= 0 && N >= 0, "layerscale_apply: negative size");
  VITMI_CHECK_ARG(N % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= N && ldy >= N,
                  "layerscale_apply: N and leading dims must be multiples of 4");
  VITMI_CHECK_ARG(aligned_to(x, 16) && aligned_to(gamma, 16) && aligned_to(y, 8), "layerscale_apply: alignment");
  if (M == 0 || N == 0) return VITMI_OK;
  const bool f32 = y_dtype == VITMI_F32;
  launch(f32 ? untyped(layerscale_apply_kernel<float>) : untyped(layerscale_apply_kernel<bf16>),
         dim3(grid_cap(M * (N / 4))), dim3(256), (hipStream_t)stream, 0, (f32 ? 8.0 : 6.0) * M * N, M, N, x, ldx, gamma,
         y, ldy);
  VITMI_LAUNCH_CHECK("layerscale_apply");
  return VITMI_OK;
}

extern "C" size_t vitmi_layerscale_dgamma_workspace_size(int64_t M, int64_t N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)dgamma_splits(M, N) * N * sizeof(float);
}

extern "C" int vitmi_layerscale_dgamma(int64_t M, int64_t N, const float* dy, int64_t lddy, const float* x,
                                       int64_t ldx, float* dgamma, void* workspace, size_t ws_bytes,
                                       vitmi_stream_t stream) {
  VITMI_CHECK_ARG(dy && x && dgamma, "layerscale_dgamma: null pointer");
  VITMI_CHECK_ARG(M >= 0 && N >= 0, "layerscale_dgamma: negative size");
  VITMI_CHECK_ARG(N % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddy >= N && ldx >= N,
                  "layerscale_dgamma: N and leading dims must be multiples of 4");
  VITMI_CHECK_ARG(aligned_to(dy, 16) && aligned_to(x, 16), "layerscale_dgamma: alignment");
  if (M == 0 || N == 0) return VITMI_OK;
  VITMI_CHECK_ARG(workspace && aligned_to(workspace, 16) && ws_bytes >= vitmi_layerscale_dgamma_workspace_size(M, N),
                  "layerscale_dgamma: workspace too small");
  const int Z = dgamma_splits(M, N);
  const int64_t rows_per = (M + Z - 1) / Z;
  const hipStream_t s = (hipStream_t)stream;
  launch(layerscale_dgamma_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)Z), dim3(256), s, 2.0 * M * N,
         8.0 * M * N, M, N, dy, lddy, x, ldx, (float*)workspace, rows_per);
  VITMI_LAUNCH_CHECK("layerscale_dgamma");
  return fold_rows((const float*)workspace, Z, N, N, dgamma, s);
}
