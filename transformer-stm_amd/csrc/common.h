// Shared device/host helpers for the gfx950 (CDNA4) kernels of libvitmi.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include "../../include/vitmi.h"

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

namespace vitmi {

// ---------------------------------------------------------------- host side
void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define VITMI_CHECK_ARG(cond, ...)                                   \
  do {                                                               \
    if (!(cond)) return ::vitmi::fail(VITMI_ERR_INVALID, __VA_ARGS__); \
  } while (0)

#define VITMI_HIP_CHECK(call, what)                                           \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess)                                                     \
      return ::vitmi::fail(VITMI_ERR_HIP, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

#define VITMI_LAUNCH_CHECK(what)                                              \
  do {                                                                        \
    hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess)                                                     \
      return ::vitmi::fail(VITMI_ERR_HIP, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

// ---------------------------------------------------------------- conversions
__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16 x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16 from_f32<bf16>(float x) { return (bf16)x; }

// ---------------------------------------------------------------- e4m3 (the bf16f8 knob)
// VITMI_BF16F8 operands (the precision knob's cheaper form): x = hi + lo, hi = bf16(x); the row
// carries hi (bf16) and two OCP e4m3 parts, hi8 = e4m3(hi) and lo8 = e4m3(lo * 2^9), so the two
// correction products hi.lo + lo.hi run as ONE block-scaled fp8 product (the GEMM's fp8 K-steps,
// scale 2^-9 on the weight operand).  lo = x - hi is exact in fp32, at most half a bf16 ulp:
// |lo| <= 2^(e-8) for 2^e <= |x| < 2^(e+1), so lo8 = lo * 2^9 <= 2^(e+1) <= 2|x|.  The fixed scales
// bound where the corrections hold (tools/precision_emulate_fp8.py): e4m3 saturates at
// +-448, so lo8 can clip once |x| > 224 and hi8 once |x| > 448, and past that the product falls back
// to roughly plain-bf16 accuracy; at the small end hi8 is subnormal below |x| = 2^-6 and lo8 below
// |lo| = 2^-15, where those terms lose relative precision (but weigh < 2^-6 of a unit operand).
// tests/test_gpu_f8.py bounds the GEMM error inside the range (|x| up to ~200) and shows the
// fallback to bf16 accuracy past it.
// The e4m3 part (2K bytes after the K bf16 of hi) interleaves per 64 k: block j = [hi8 of k
// 64j..64j+63 | lo8 of the same k] for an A operand, [lo8 | hi8] for a weight, so one 128-B GEMM
// K-step pairs hi8.lo8 and lo8.hi8 of the same 64 k, and a producer's 64-column tile leaves as
// whole 128-B lines (K % 64 == 0).
__host__ __device__ constexpr int64_t f8_off(int64_t c) { return (c >> 6) * 128 + (c & 63); }
constexpr float F8_LO_SCALE = 512.f;
constexpr int F8_E8M0_ONE = 127, F8_E8M0_LO = 127 - 9;   // E8M0 scales 1 and 2^-9
// four floats -> four OCP e4m3 bytes (RNE; saturated to +-448 first: the conversion itself would
// give NaN past the range), little-endian in one dword
__device__ __forceinline__ uint32_t e4m3x4(float a, float b, float c, float d) {
  a = __builtin_amdgcn_fmed3f(a, 448.f, -448.f);
  b = __builtin_amdgcn_fmed3f(b, 448.f, -448.f);
  c = __builtin_amdgcn_fmed3f(c, 448.f, -448.f);
  d = __builtin_amdgcn_fmed3f(d, 448.f, -448.f);
  int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  return (uint32_t)v;
}
// hi (bf16), hi8 and lo8 (dwords of 4 e4m3) of four fp32 values
__device__ __forceinline__ void split_f8(f32x4 v, bf16x4& hi, uint32_t& hi8, uint32_t& lo8) {
  f32x4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hi[e] = (bf16)v[e];
    h[e] = (float)hi[e];
    l[e] = (v[e] - h[e]) * F8_LO_SCALE;
  }
  hi8 = e4m3x4(h[0], h[1], h[2], h[3]);
  lo8 = e4m3x4(l[0], l[1], l[2], l[3]);
}

// exact-erf GELU (tf.nn.gelu default, models/CvT(Par).py:254) and its derivative
__device__ __forceinline__ float gelu_f(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}
__device__ __forceinline__ float gelu_grad_f(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// ---------------------------------------------------------------- dropout mask
// Keep-mask of dropout (layers.Dropout, models/CvT(Par).py:189,255,257; Keras rate 0.1 in
// training): a counter hash of (seed, site, row, col) built from murmur3's 32-bit finaliser,
// keep iff hash >= thresh with thresh = round(p * 2^32).  Kept elements are scaled by
// 1/(1-p).  The mask is regenerated wherever it is needed (forward epilogue, backward copy)
// and never stored; oracle/vit_ref.py restates the same function bit for bit.
__host__ __device__ inline uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t drop_row_key(uint32_t seed, uint32_t site, uint32_t row) {
  return fmix32(seed ^ (site * 0x9E3779B1u) ^ fmix32(row + 0x7F4A7C15u));
}
__host__ __device__ inline uint32_t drop_hash(uint32_t row_key, uint32_t col) {
  return fmix32(row_key ^ (col * 0x85EBCA77u));
}

// ---------------------------------------------------------------- drop path (stochastic depth)
// One keep decision per sample of a drop-path site: sample b is kept iff drop_hash(drop_row_key(seed,
// site, b), 0) >= thresh (the dropout hash at row = sample, col = 0; include/vitmi.h).  Row r of an
// [M, .] operand belongs to sample r / S.  The kernels divide by a multiply: with magic =
// floor(2^32 / S) + 1 = (2^32 + e) / S, 1 <= e <= S, mulhi(r, magic) = floor(r / S + r e / (S 2^32)),
// which is floor(r / S) whenever r e < 2^32; r < M and e <= S, so M * S <= 2^32 is enough
// (path_map_exact, the entry points' host check).  S = 1 has no 32-bit magic and maps r to itself.
__host__ __device__ inline bool path_keep(uint32_t seed, uint32_t site, uint32_t sample, uint32_t thresh) {
  return drop_hash(drop_row_key(seed, site, sample), 0u) >= thresh;
}
inline uint32_t path_magic(uint32_t S) { return S < 2 ? 0u : (uint32_t)((1ull << 32) / S) + 1u; }
inline bool path_map_exact(int64_t M, int64_t S) { return M <= 0 || (S >= 1 && S <= (1ll << 32) / M); }
__device__ __forceinline__ uint32_t path_sample(uint32_t row, uint32_t S, uint32_t magic) {
  return S == 1 ? row : __umulhi(row, magic);
}

// ---------------------------------------------------------------- reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------- buffer resources
// A raw buffer descriptor: loads past `bytes` return 0 (the hardware range check),
// which is how ragged M/N/reduction edges are zero-filled without branches.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ uint32_t clamp_bytes(int64_t b) {
  return b <= 0 ? 0u : (b > 0x7fffffff ? 0x7fffffffu : (uint32_t)b);
}

// Algorithmic work of one kernel launch (flops = 2 x MACs of its dense contractions, bytes =
// the HBM bytes its operands must move at least once), accumulated per kernel while
// vitmi_stats_enable(1) is on (abi.cpp): bench.py joins it with a rocprofv3 kernel trace of
// the same run to report per-kernel TFLOP/s and GB/s.  Off (one branch) otherwise.
extern bool g_stats_on;
void stat_record(const void* kernel, double flops, double bytes);
#define VITMI_STAT(kernel, flops, bytes)                                                     \
  do {                                                                                      \
    if (::vitmi::g_stats_on) ::vitmi::stat_record((const void*)(kernel), (double)(flops), (double)(bytes)); \
  } while (0)

// ---------------------------------------------------------------- host launch layer
// Every kernel launch of the library: one hipLaunchKernelGGL and its VITMI_STAT record, both from the
// same kernel argument.  A kernel that records no work is launched with `no_stat` in place of the flops
// and bytes.  Neither form checks the launch: VITMI_LAUNCH_CHECK returns from its caller, so it stays
// in the entry point.
template <typename... P, typename... A>
inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, double flops, double bytes, A... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
  VITMI_STAT(kernel, flops, bytes);
}
struct NoStat {};
constexpr NoStat no_stat{};
template <typename... P, typename... A>
inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, NoStat, A... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// A kernel seen with untyped pointer parameters, so that the instances of one template that differ
// in an operand's element type share one pointer type: a runtime dtype picks the instance (a
// conditional expression or a small table), then one launch takes it.  Only the pointee types are
// erased; the launch packs the same arguments.
template <typename T> struct untyped_param { typedef T type; };
template <typename T> struct untyped_param<T*> { typedef void* type; };
template <typename T> struct untyped_param<const T*> { typedef const void* type; };
template <typename... P>
inline auto untyped(void (*kernel)(P...)) {
  return reinterpret_cast<void (*)(typename untyped_param<P>::type...)>(kernel);
}

// blocks of a grid-stride launch: ceil(work / per_block) in [1, cap]; GRID_NO_CAP (the grid's own
// limit) for a kernel that takes one block per per_block items, whatever the work
constexpr int64_t GRID_NO_CAP = 0x7fffffff;
inline unsigned grid_cap(int64_t work, int per_block = 256, int64_t cap = 8192) {
  const int64_t g = (work + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// a null pointer (an output that is not asked for) counts as aligned
inline bool aligned_to(const void* p, uintptr_t bytes) { return (uintptr_t)p % bytes == 0; }

// compute units of the current device, looked up once; 256 (the MI355X) when the query fails (abi.cpp)
int device_cus();

// db[n] += sum_z part[z][n] in a fixed order (elementwise.hip)
int launch_colsum_finish(int64_t N, int Z, const float* part, float* db, hipStream_t s);
// out[c] += sum_r part[r * ld + c] (fixed order), launched now or, between vitmi_fold_begin and
// vitmi_fold_end on this thread, queued and launched with the other queued folds (elementwise.hip)
int fold_rows(const float* part, int64_t rows, int64_t cols, int64_t ld, float* out, hipStream_t s);

}  // namespace vitmi
