/*
 * vitmi.h — C ABI of libvitmi.so, the MI355X (gfx950 / CDNA4) ViT training path.
 *
 * Drop-in boundary.  The reference's hot path is the forward + autodiff backward
 * of its transformer stage, dispatched by Keras to TensorFlow GPU library ops
 * (SURVEY.md §2 op table).  Each entry point below replaces one such library op
 * at its call site in the reference; the Python layer (vitmi/ops.py, vitmi/modules.py)
 * mirrors the reference's layer API and calls these through ctypes.
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (the PyTorch caching
 *     allocator).  No entry point allocates, frees or synchronises the host.
 *   - Every call is stream-ordered on `stream` (a hipStream_t) and re-entrant.
 *   - Matrices are row-major with an explicit leading dimension in ELEMENTS.
 *   - Accumulating outputs (parameter gradients) are fp32 and updated with +=,
 *     the semantics of torch's .grad accumulation.
 *   - Return 0 on success, otherwise a VITMI_ERR_* code; vitmi_last_error()
 *     returns a thread-local message.  Shapes are validated on the host before
 *     any launch; there is no silent fallback path.
 */
#ifndef VITMI_H
#define VITMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vitmi_stream_t; /* hipStream_t */

enum { VITMI_OK = 0, VITMI_ERR_INVALID = 1, VITMI_ERR_HIP = 2, VITMI_ERR_UNSUPPORTED = 3, VITMI_ERR_COMM = 4 };
enum {
  VITMI_F32 = 0,
  VITMI_BF16 = 1,
  VITMI_F64 = 2,    /* comm only */
  VITMI_BF16X3 = 3, /* vitmi_layernorm_fwd's y only: bf16 rows [hi | hi | lo] of 3D columns, the
                       split-bf16 A operand of the precision knob (vitmi_split_bf16x3) */
  VITMI_BF16F8 = 4, /* the knob's cheaper form (ViTConfig dtype "bf16f8"): a row of K values is 4K
                       bytes (2K bf16 units), [hi = bf16(x) (K bf16) | OCP e4m3 part (2K bytes)],
                       the e4m3 part in 64-k blocks of 128 B, [hi8 | lo8] for an A operand
                       (activations) and [lo8 | hi8] for a weight, hi8 = e4m3(hi), lo8 =
                       e4m3((x - hi) * 2^9) (vitmi_split_bf16f8; K % 64 == 0).
                       vitmi_linear_fwd dtype (x and w both so; K % 64 == 0, N % 16 == 0): the
                       GEMM runs K/64 bf16 K-steps (hi.hi) and K/64 block-scaled fp8 K-steps
                       (hi.lo + lo.hi, v_mfma_scale_f32_16x16x128_f8f6f4): 2K-equivalent MFMA
                       work instead of bf16x3's 3K.  Also vitmi_layernorm_fwd's y dtype. */
  VITMI_BF16F8W = 5 /* the weight-side correction alone (the bf16f8 knob's qkv GEMM): a row of K values
                       is 3K bytes (1.5K bf16 units), [hi = bf16(x) (K bf16) | one OCP e4m3 byte per
                       k (K bytes)], the byte hi8 = e4m3(hi) for an A operand (activations) and lo8 =
                       e4m3((x - hi) * 2^9) for a weight (vitmi_split_bf16f8 patterns 2 / 3; K % 128
                       == 0).  vitmi_linear_fwd dtype (x and w both so): K/64 bf16 K-steps (hi.hi) and
                       K/128 block-scaled fp8 K-steps (hi.lo_w only): 1.5K-equivalent work.  The qkv
                       GEMM's error is its weight rounding's (q and k of every token move together);
                       the activation side's averages out (tools/precision_sides.py).  Also
                       vitmi_layernorm_fwd's y dtype (A-operand rows). */
};

/* GEMM epilogues (all apply `bias` (fp32, may be NULL) first where it applies) */
enum {
  VITMI_EPI_STORE = 0,     /* C = acc + bias                                        */
  VITMI_EPI_BIAS_GELU = 1, /* u = acc + bias: C = gelu(u), aux = gelu'(u) (saved)     */
  VITMI_EPI_RESIDUAL = 2,  /* C(f32) = residual(f32) + acc + bias                    */
  VITMI_EPI_DGELU = 3,     /* C = acc * aux   (aux = gelu'(u) from BIAS_GELU)        */
  VITMI_EPI_ACCUM = 4      /* C(f32) += acc                                          */
};
/* OR'ed into BIAS_GELU / DGELU (bf16 operands only): aux is kept in the library's tile-native
 * layout instead of a row-major [M][N] array -- vitmi_aux_tiled_bytes(M, N) bytes, written by a
 * BIAS_GELU call and read by a DGELU call of the same M x N output, opaque to the caller.  The
 * GEMM epilogues then store and load it straight from the accumulator registers (no LDS
 * transpose): the fc1 forward / fc2 dgrad pair of the ViT MLP (models/CvT(Par).py:253-258). */
#define VITMI_EPI_AUX_TILED 0x100
size_t vitmi_aux_tiled_bytes(int64_t rows, int64_t cols);
/* OR'ed into BIAS_GELU of vitmi_linear_fwd (bf16 operands and output; the precision knob,
 * ViTConfig dtype "bf16x3"): y is bf16 [M][3N], each row [hi | hi | lo] of the fp32 gelu(u)
 * (hi = bf16(a), lo = bf16(a - hi): the split A operand of the next GEMM, vitmi_split_bf16x3
 * pattern 0); aux = gelu'(u) as for BIAS_GELU. */
#define VITMI_EPI_SPLIT_X3 0x200
/* OR'ed into BIAS_GELU of vitmi_linear_fwd with dtype VITMI_BF16F8 (y_dtype VITMI_BF16; N % 64 == 0):
 * y is [M][2N] bf16 units, each row the VITMI_BF16F8 A-operand layout of gelu(u); aux as for BIAS_GELU. */
#define VITMI_EPI_SPLIT_F8 0x400

enum { VITMI_LOSS_CE = 0, VITMI_LOSS_MSE = 1 };

int vitmi_version(void);
/* "<sources>-<flags>": 16 hex digits of the content hash of the sources the library was built
 * from (csrc/ + this header), then 8 of the hash of its compiler command line
 * (vitmi_build_flags); __graft_entry__ compares the first part with the tree it runs in, so a
 * stale .so is caught, and a variant built with other flags or -D switches has another id */
const char* vitmi_build_id(void);
const char* vitmi_build_flags(void);
const char* vitmi_last_error(void);
/* number of hipDevice compute units seen by the library (0 on error) */
int vitmi_device_cus(void);
/* Per-kernel algorithmic work accounting (host side, off by default): while enabled every
 * launch adds its 2 x MAC flops and minimum HBM bytes to its kernel's entry (keyed by the
 * mangled device symbol).  Enabling clears the table.  bench.py joins these with a rocprofv3
 * kernel trace of the same run (per-kernel TFLOP/s, GB/s). */
int vitmi_stats_enable(int on);
int vitmi_stats_count(void);
int vitmi_stats_get(int i, char* name, int name_len, int64_t* calls, double* flops, double* bytes);
/* ROCTx ranges (rocprofv3 --marker-trace): off by default; enabling binds the ROCm marker
 * library at run time (VITMI_ERR_UNSUPPORTED if absent).  vitmi/trace.py wraps the training
 * step's forward / backward / all-reduce / optimizer phases in them. */
int vitmi_trace_enable(int on);
int vitmi_trace_push(const char* name);
int vitmi_trace_pop(void);

/* ---------------------------------------------------------------------------
 * Generic MFMA GEMM:  C[M,N] (op)= sum_k A(m,k) * B(k,n)
 *   a_kmajor=1: A stored [M][lda] (k contiguous);  0: A stored [K][lda] (m contiguous)
 *   b_kmajor=1: B stored [N][ldb] (k contiguous);  0: B stored [K][ldb] (n contiguous)
 *   dtype: operand type (VITMI_BF16 -> v_mfma_f32_16x16x32_bf16, VITMI_F32 -> v_mfma_f32_16x16x4_f32)
 *   c_dtype: output type; aux (the saved GELU derivative gelu'(u)) has the operand dtype.
 *   BIAS_GELU on bf16 operands writes bf16 (c_dtype VITMI_F32 is rejected).
 *   k-major operands need K % 64 == 0 (bf16) / K % 32 == 0 (f32); ragged M/N and a
 *   ragged reduction over m-major operands are zero-filled by the buffer range check.
 * Replaces the reference's Dense/EinsumDense MatMul and their autodiff transposes
 * (models/CvT(Par).py:132-134,137,142,188,254,256).
 */
int vitmi_gemm(int dtype, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K,
               const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
               int c_dtype, int epilogue, const float* bias, void* aux, int64_t ldaux,
               const float* residual, int64_t ldr, void* workspace, size_t ws_bytes,
               vitmi_stream_t stream);
/* Kernel selection (process-wide): 0 = auto (default), 1 = always the 128x128 tile kernel,
 * 2 = always the 256x256 8-wave bf16 kernel where the dtype allows, 3 = as 2 on an 8-block
 * persistent grid (each block walks many tiles).  For tests/diagnostics. */
int vitmi_gemm_set_policy(int policy);
size_t vitmi_gemm_workspace_size(int dtype, int a_kmajor, int b_kmajor, int64_t M, int64_t N,
                                 int64_t K, int epilogue);

/* Linear layer y = x W^T + b  (keras layers.Dense, models/CvT(Par).py:132-134,142,254,256;
 * torch nn.Linear in old_codes/MS_CvT.py:63-65,116-121).  x [M,K], W [N,K] -> y [M,N]. */
/* workspace: optional (NULL/0 allowed).  With vitmi_linear_*_workspace_size() bytes the
 * persistent bf16 GEMM splits the tiles of an under-filled last round over K (fp32 partials
 * in the workspace, finished by a fix-up kernel): same results up to fp32 summation order. */
int vitmi_linear_fwd(int dtype, int64_t M, int64_t N, int64_t K, const void* x, const void* w,
                     const float* bias, void* y, int y_dtype, int epilogue, void* aux,
                     const float* residual, void* workspace, size_t ws_bytes,
                     vitmi_stream_t stream);
size_t vitmi_linear_fwd_workspace_size(int dtype, int64_t M, int64_t N, int64_t K);
/* dx[M,K] = dy[M,N] W[N,K]   (epilogue STORE or DGELU with aux = gelu'(u) [M,K]) */
int vitmi_linear_dgrad(int dtype, int64_t M, int64_t N, int64_t K, const void* dy, const void* w,
                       void* dx, int dx_dtype, int epilogue, const void* aux, void* workspace,
                       size_t ws_bytes, vitmi_stream_t stream);
size_t vitmi_linear_dgrad_workspace_size(int dtype, int64_t M, int64_t N, int64_t K);
/* dW[N,K] (f32) += dy[M,N]^T x[M,K]; uses split-K over M with fp32 partial slabs */
int vitmi_linear_wgrad(int dtype, int64_t M, int64_t N, int64_t K, const void* dy, const void* x,
                       float* dw, void* workspace, size_t ws_bytes, vitmi_stream_t stream);
/* Linear dgrad with the bias gradient of its OUTPUT fused: dx = dy W (optionally * aux, DGELU)
 * and db[k] += sum_m dx[m][k] (fp32).  The bias of the layer whose INPUT gradient dx is: for
 * the MLP, du = (g W2) * gelu'(u) is fc1's output gradient, so db = fc1's bias gradient
 * (models/CvT(Par).py:254; Keras Dense bias).  On the gemm256 DGELU path the column sums come
 * from the epilogue registers (one fp32 partial row per 128 output rows, folded in a fixed
 * order), elsewhere from a second pass over dx.  workspace >= vitmi_linear_dgrad_bias_workspace_size. */
size_t vitmi_linear_dgrad_bias_workspace_size(int dtype, int64_t M, int64_t N, int64_t K);
int vitmi_linear_dgrad_bias(int dtype, int64_t M, int64_t N, int64_t K, const void* dy, const void* w, void* dx,
                            int dx_dtype, int epilogue, const void* aux, float* db, void* workspace, size_t ws_bytes,
                            vitmi_stream_t stream);

size_t vitmi_linear_wgrad_workspace_size(int dtype, int64_t M, int64_t N, int64_t K);
/* Grouped weight gradients over ONE row count M: for p < n (n <= 4), dW_p[N[p], K[p]] (f32) +=
 * dy_p[M, N[p]]^T x_p[M, K[p]], dy_p rows of pitch lddy[p] and x_p of pitch ldx[p] elements (NULL
 * or 0: dense).  The four weight gradients of a transformer block (models/CvT(Par).py:253-258,
 * 132-142: fc2, fc1, out-projection, qkv) in one split-K launch over all their tiles and one
 * reduction launch (bf16; other dtypes and shapes run one vitmi_linear_wgrad-equivalent GEMM per
 * problem).  workspace >= vitmi_linear_wgrad_group_workspace_size(dtype, n, M, N, K). */
int vitmi_linear_wgrad_group(int dtype, int n, int64_t M, const int64_t* N, const int64_t* K,
                             const void* const* dy, const int64_t* lddy, const void* const* x,
                             const int64_t* ldx, float* const* dw, void* workspace, size_t ws_bytes,
                             vitmi_stream_t stream);
size_t vitmi_linear_wgrad_group_workspace_size(int dtype, int n, int64_t M, const int64_t* N,
                                               const int64_t* K);
/* db[N] (f32) += sum_m dy[m, n]  (dy [M][ldy] of `dtype`).
 * Preconditions (VITMI_ERR_INVALID otherwise, nothing launched): dtype VITMI_F32 or VITMI_BF16; ldy >= N;
 * dy and db aligned to their element; workspace >= vitmi_bias_grad_workspace_size(M, N).  A 16-byte
 * aligned dy with N % 8 == 0 and ldy % 8 == 0 takes the vector kernel, anything else the one-column-
 * per-thread kernel.  M == 0 or N == 0 leaves db untouched. */
int vitmi_bias_grad(int dtype, int64_t M, int64_t N, const void* dy, int64_t ldy, float* db,
                    void* workspace, size_t ws_bytes, vitmi_stream_t stream);
size_t vitmi_bias_grad_workspace_size(int64_t M, int64_t N);

/* ---------------------------------------------------------------------------
 * LayerNorm over the last dim D (layers.LayerNormalization, models/CvT(Par).py:248,328;
 * old_codes/MS_CvT.py:39-45).  x is fp32 [M][ldx]; y [M][ldy] of y_dtype; mean/rstd fp32 [M].
 * y_dtype VITMI_BF16X3: y is bf16 [M][ldy >= 3D], each row [hi | hi | lo] of the fp32 result.
 * y_dtype VITMI_BF16F8: y is [M][ldy >= 2D] bf16 units, each row the VITMI_BF16F8 A-operand layout
 *   [hi | e4m3 part in 64-column blocks hi8 | lo8]; D % 64 == 0.
 * y_dtype VITMI_BF16F8W: y is [M][ldy >= 1.5D] bf16 units, each row [hi | hi8] (one e4m3 byte per
 *   column); D % 128 == 0.
 * Preconditions (VITMI_ERR_INVALID otherwise, nothing launched): D % 4 == 0, 4 <= D <= 2048; ldx and
 * ldy multiples of 4 (elements of x, resp. bf16 / fp32 units of y), ldx >= D and ldy >= the row width
 * above; y_dtype one of the five named; x, gamma, beta and an fp32 y 16-byte aligned, every bf16-unit
 * y 8-byte aligned (every access is a 4-element vector).  M == 0 returns VITMI_OK and writes nothing.
 */
int vitmi_layernorm_fwd(int64_t M, int D, const float* x, int64_t ldx, const float* gamma,
                        const float* beta, float eps, void* y, int y_dtype, int64_t ldy,
                        float* mean, float* rstd, vitmi_stream_t stream);
/* dx = dres + LN'(dy); optional low-precision copy dx_lp (bf16); dgamma/dbeta += (fp32);
 * optional dxsum[D] += column sums of dx (the bias gradient of the Dense layer whose output
 * gradient dx is: fused so that gradient is never re-read). NULL pointers skip outputs.
 * Preconditions (VITMI_ERR_INVALID otherwise, nothing launched): D as in the forward; dy_dtype
 * VITMI_F32 or VITMI_BF16 (the split forms are forward outputs only); lddy, ldx, lddx, and ldres /
 * lddx_lp when dres / dx_lp is given, multiples of 4 and >= D; x, gamma, dres, dx and an fp32 dy
 * 16-byte aligned, a bf16 dy and dx_lp 8-byte aligned; workspace >=
 * vitmi_layernorm_bwd_workspace_size(M, D).  M == 0 returns VITMI_OK and writes nothing. */
int vitmi_layernorm_bwd(int64_t M, int D, const void* dy, int dy_dtype, int64_t lddy,
                        const float* x, int64_t ldx, const float* mean, const float* rstd,
                        const float* gamma, const float* dres, int64_t ldres, float* dx,
                        int64_t lddx, void* dx_lp, int64_t lddx_lp, float* dgamma, float* dbeta,
                        float* dxsum, void* workspace, size_t ws_bytes, vitmi_stream_t stream);
size_t vitmi_layernorm_bwd_workspace_size(int64_t M, int D);
/* ---------------------------------------------------------------------------
 * QK-norm: LayerNorm over the head dimension of the queries and keys before QK^T (ViT-22B; timm's
 * qk_norm=True with norm_layer=LayerNorm, blocks.i.attn.q_norm / k_norm).  qkv is [M][ld >= 3*H*dh] of
 * dtype (VITMI_F32 or VITMI_BF16) in the attention layout (q | k | v column blocks, head h at h*dh),
 * dh = 64, 1 <= H <= 32.  gamma_* / beta_* are fp32 [dh], one pair for q and one for k, shared by all
 * heads.  mean / rstd are fp32 [M][2H]: column j < H is q head j, column H + j is k head j.
 *
 * vitmi_qknorm_fwd: out [M][ldo >= 3*H*dh] (same dtype) gets LN(q head; gamma_q, beta_q, eps) and
 *   LN(k head; gamma_k, beta_k, eps) -- mean, variance about the computed mean, rsqrtf, (x - mu) * rs *
 *   g + b in fp32, one round-to-nearest store -- and the v block bit for bit, so the attention entry
 *   points take `out` unchanged.  out must not alias qkv: the backward reads the pre-norm values.
 * vitmi_qknorm_bwd: qkv is the forward's INPUT (pre-norm), mean / rstd its statistics.  dqkv [M][ldd]
 *   arrives holding the gradient of `out` (the attention backward's output); its q and k blocks are
 *   replaced in place by rs * (gy - mean(gy) - xhat * mean(gy * xhat)), gy = dy * gamma, rounded once to
 *   dtype; the v block is not written.  dgamma_* / dbeta_* [dh] += the sums over rows and heads of
 *   dy * xhat / dy; dbias [3*H*dh] += the column sums of the finished dqkv (the qkv bias gradient: for q
 *   and k the stored, rounded values, for v the columns as given).  Each of the five may be NULL.  The
 *   sums are per-thread and per-block partials in the workspace (>= vitmi_qknorm_bwd_workspace_size(M,
 *   H) bytes, either dtype) finished by the fixed-order fold (queued between vitmi_fold_begin and
 *   vitmi_fold_end): no atomics, bitwise reproducible.
 * Preconditions (VITMI_ERR_INVALID otherwise, nothing launched): dtype one of the two; dh == 64; H in
 * [1, 32]; ld, ldo, ldd >= 3*H*dh and multiples of 8 (bf16) / 4 (fp32); qkv, out, dqkv, gamma, beta and
 * the workspace 16-byte aligned (every access is a 16-byte vector); no required pointer NULL; out !=
 * qkv; the workspace large enough.  M == 0 returns VITMI_OK and writes nothing. */
int vitmi_qknorm_fwd(int dtype, int64_t M, int H, int dh, const void* qkv, int64_t ld,
                     const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                     float eps, void* out, int64_t ldo, float* mean, float* rstd, vitmi_stream_t stream);
size_t vitmi_qknorm_bwd_workspace_size(int64_t M, int H);
int vitmi_qknorm_bwd(int dtype, int64_t M, int H, int dh, const void* qkv, int64_t ld,
                     const float* mean, const float* rstd, const float* gamma_q, const float* gamma_k,
                     void* dqkv, int64_t ldd, float* dgamma_q, float* dbeta_q, float* dgamma_k, float* dbeta_k,
                     float* dbias, void* workspace, size_t ws_bytes, vitmi_stream_t stream);
/* ---------------------------------------------------------------------------
 * Multi-head scaled-dot-product attention (layers.MultiHeadAttention called (q, v, k),
 * models/CvT(Par).py:137,185; einsum-softmax-einsum old_codes/MS_CvT.py:202-207).
 * qkv: [B*N][3*H*dh] token-major (q | k | v column blocks, head h at h*dh); o: [B*N][H*dh];
 * lse: fp32 [B*H][N] (natural-log softmax normaliser per query, saved for backward).
 * dh must be 64.  dtype selects bf16 MFMA (VITMI_BF16) or fp32 (VITMI_F32) kernels.
 */
int vitmi_attention_fwd(int dtype, int B, int N, int H, int dh, float scale, const void* qkv,
                        void* o, float* lse, vitmi_stream_t stream);
/* The precision knob's attention forward (bf16 q, k, v; ViTConfig dtype "bf16x3"): as
 * vitmi_attention_fwd(VITMI_BF16, ...) -- o (bf16 [B*N][H*dh]) and lse bit for bit -- plus o3,
 * bf16 [B*N][3*H*dh], each row [hi | hi | lo] of the fp32 output (the out-projection GEMM's
 * split A operand, vitmi_split_bf16x3 pattern 0).  N <= 256 (the whole-sequence kernel). */
int vitmi_attention_fwd_x3(int B, int N, int H, int dh, float scale, const void* qkv, void* o, void* o3,
                           float* lse, vitmi_stream_t stream);
/* As vitmi_attention_fwd_x3 for the VITMI_BF16F8 knob: o8 is [B*N][2*H*dh] bf16 units, each row the
 * VITMI_BF16F8 A-operand layout [hi | hi8 | lo8] of the fp32 output. */
int vitmi_attention_fwd_f8(int B, int N, int H, int dh, float scale, const void* qkv, void* o, void* o8,
                           float* lse, vitmi_stream_t stream);
int vitmi_attention_bwd(int dtype, int B, int N, int H, int dh, float scale, const void* qkv,
                        const void* o, const void* dout, const float* lse, void* dqkv,
                        void* workspace, size_t ws_bytes, vitmi_stream_t stream);
size_t vitmi_attention_bwd_workspace_size(int B, int N, int H);
/* Kernel selection (process-wide; tests): 0 = auto (bf16, N <= 224: the single-pass backward, dQ,
 * dK and dV in one persistent kernel), 1 = always the streamed (64-key LDS-tiled) kernels, 2 = the
 * whole-sequence kernels' 32-query-per-wave forward and dQ forms and the two-kernel backward (auto
 * runs their 64-query forms, bitwise equal), 3 = auto's forward with the two-kernel backward
 * (64-query dQ, then dK/dV).  Returns the previous policy. */
int vitmi_attention_set_policy(int policy);
/* vitmi_attention_bwd plus the qkv bias gradient: dbias[3*H*dh] += column sums of dqkv (the
 * q/k/v Dense biases, models/CvT(Par).py:132-134).  On the bf16 paths the sums come from the
 * backward kernels' output images (per (batch, head) block on the whole-sequence path,
 * N <= 256, per (batch, head, 128-row block) on the streamed one, then a fixed-order fold); the
 * fp32 paths take a second pass over dqkv. */
size_t vitmi_attention_bwd_bias_workspace_size(int B, int N, int H);
int vitmi_attention_bwd_bias(int dtype, int B, int N, int H, int dh, float scale, const void* qkv, const void* o,
                             const void* dout, const float* lse, void* dqkv, float* dbias, void* workspace,
                             size_t ws_bytes, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Patch embedding Conv2D(k=P, s=P) as a GEMM (models/CvT(Par).py:203-212;
 * old_codes/MS_CvT.py:352-361): im2col of the fp32 NCHW images into
 * patches [B*(S/P)^2][C*P*P] of `dtype` (column order c, kh, kw = the conv weight's).
 * Limits: S % P == 0, P % 4 == 0, C*P*P <= 4096 (one thread per 4 columns of a patch row).
 * dtype is VITMI_F32 or VITMI_BF16 (any other is refused: the kernels write nothing else); B >= 0
 * (B == 0 does nothing), C > 0, S > 0; img 16-byte aligned, patches 16-byte (fp32) or 8-byte (bf16)
 * aligned.
 */
int vitmi_patch_im2col(int dtype, int B, int C, int S, int P, const float* img, void* patches,
                       vitmi_stream_t stream);
/* x[b][0] = cls + pos[0];  x[b][1+p] = tok[b*np+p] + pos[1+p]   (cls/pos may be NULL).
 * B >= 0, np >= 0, D > 0 and D % 4 == 0; every pointer given is 16-byte aligned. */
int vitmi_tokens_assemble(int B, int np, int D, const float* tok, const float* cls,
                          const float* pos, float* x, vitmi_stream_t stream);
/* backward of assemble: dtok (f32, and optional bf16 copy) = dx[:,1:];  dpos += sum_b dx,
 * dcls += sum_b dx[:,0]   (NULL pointers skip that output).  The sums run over b = 0, 1, ... in
 * order from 0 and are added to what dpos / dcls hold (bitwise reproducible).  B >= 0, np >= 0,
 * D > 0 and D % 4 == 0; every pointer given is 16-byte aligned (dtok_lp: 8-byte). */
int vitmi_tokens_assemble_bwd(int B, int np, int D, const float* dx, float* dtok, void* dtok_lp,
                              float* dcls, float* dpos, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Per-op entry points under the names of SURVEY.md §8(b) (csrc/boundary.cpp).  Each composes
 * the kernel-level entry points above on the same stream (bit-identical results) and takes a
 * caller-owned workspace of at least the queried size.
 *
 * vitmi_patch_embed_fwd replaces ConvEmbed.call's Conv2D (models/CvT(Par).py:211-217) plus the
 * block's cls concat (:264-268) and the position embedding:
 *   patches (out, saved for the backward) = im2col(img) [B*np][C*P*P] of dtype, np = (S/P)^2;
 *   x (out, fp32 [B][np+1][D]) = [cls ; patches W^T + bias] + pos   (cls/pos/bias may be NULL);
 *   w: [D][C*P*P] of dtype (the conv weight flattened).
 * vitmi_patch_embed_bwd: dW += ..., dbias += ..., dcls += ..., dpos += ... from dx (NULL skips).
 * dtype is VITMI_F32 or VITMI_BF16 in all of these (and in the _keep forms); any other is refused and
 * its workspace query returns 0: the split operand dtypes take an fp32 im2col followed by a split. */
size_t vitmi_patch_embed_fwd_workspace_size(int dtype, int B, int C, int S, int P, int D);
int vitmi_patch_embed_fwd(int dtype, int B, int C, int S, int P, int D, const float* img, const void* w,
                          const float* bias, const float* cls, const float* pos, void* patches, float* x,
                          void* workspace, size_t ws_bytes, vitmi_stream_t stream);
size_t vitmi_patch_embed_bwd_workspace_size(int dtype, int B, int C, int S, int P, int D);
int vitmi_patch_embed_bwd(int dtype, int B, int C, int S, int P, int D, const float* dx, const void* patches,
                          float* dw, float* dbias, float* dcls, float* dpos, void* workspace, size_t ws_bytes,
                          vitmi_stream_t stream);
/* Autodiff of layers.Dense (models/CvT(Par).py:132-134,142,188,254,256): dx = dy W (dx_dtype,
 * NULL skips), dW += dy^T x, db += column sums of dy (fp32, NULL skips).  dy/x/w of dtype. */
size_t vitmi_linear_bwd_workspace_size(int dtype, int64_t M, int64_t N, int64_t K);
int vitmi_linear_bwd(int dtype, int64_t M, int64_t N, int64_t K, const void* dy, const void* x, const void* w,
                     void* dx, int dx_dtype, float* dw, float* db, void* workspace, size_t ws_bytes,
                     vitmi_stream_t stream);
/* Losses, mean over the batch: softmax cross-entropy (BASELINE configs, target int64 [B]) and
 * Keras 'mean_squared_error' (models/CvT(Par).py:464-466, target fp32 [B][C]).  _fwd writes
 * the scalar loss, _bwd d(loss)/d(logits) [B][C] (upstream gradient 1). */
int vitmi_xent_fwd(int B, int C, const float* logits, const int64_t* target, float* loss, vitmi_stream_t stream);
int vitmi_xent_bwd(int B, int C, const float* logits, const int64_t* target, float* dlogits, vitmi_stream_t stream);
int vitmi_mse_fwd(int B, int C, const float* pred, const float* target, float* loss, vitmi_stream_t stream);
int vitmi_mse_bwd(int B, int C, const float* pred, const float* target, float* dpred, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Head (layers.Dense(num_classes) on LN(cls), models/CvT(Par).py:326-329,350) and loss
 * (compile(loss='mean_squared_error') :464-466; softmax-CE for >=2 classes).
 * y: fp32 [B][ldy]; W fp32 [C][D].  Both calls need B > 0, C > 0, D > 0 and ldy >= D.
 */
int vitmi_head_fwd(int B, int D, int C, const float* y, int64_t ldy, const float* w,
                   const float* b, float* logits, vitmi_stream_t stream);
int vitmi_head_bwd(int B, int D, int C, const float* dlogits, const float* y, int64_t ldy,
                   const float* w, float* dy, float* dw, float* db, vitmi_stream_t stream);
/* loss = mean over batch; dlogits = d loss / d logits.  target: int64 [B] (CE) or f32 [B][C] (MSE).
 * Either output may be NULL (not both).  A CE label outside [0, C) matches no class (as in
 * vitmi_softmax_xent): the row's loss is its log-sum-exp, its gradient softmax / B, and no logit is
 * read at the label. */
int vitmi_loss_fwd_bwd(int kind, int B, int C, const float* logits, const void* target,
                       float* loss, float* dlogits, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Dropout (layers.Dropout, models/CvT(Par).py:189 after the out-projection, :255 after the
 * GELU, :257 after fc2; Keras rate 0.1, active in training only).  Element (row, col) of
 * dropout site `site` is kept iff vitmi_dropout_hash(seed, site, row, col) >= thresh, with
 * thresh = round(p * 2^32), and kept values are scaled by `scale` = 1/(1-p).  The mask is a
 * pure function of its coordinates: it is regenerated in the backward, never stored.
 */
uint32_t vitmi_dropout_hash(uint32_t seed, uint32_t site, uint32_t row, uint32_t col);
/* vitmi_linear_fwd with the dropout fused into the epilogue:
 *   BIAS_GELU: y = gelu(u) * keep * scale, aux = gelu'(u) * keep * scale (so the DGELU
 *              backward of the dropped activation needs no mask);
 *   RESIDUAL:  y = residual + (acc + bias) * keep * scale.   (x, W k-major as in linear_fwd) */
int vitmi_linear_fwd_dropout(int dtype, int64_t M, int64_t N, int64_t K, const void* x,
                             const void* w, const float* bias, void* y, int y_dtype, int epilogue,
                             void* aux, const float* residual, void* workspace, size_t ws_bytes,
                             uint32_t seed, uint32_t site, uint32_t thresh, float scale,
                             vitmi_stream_t stream);
/* y[M][ldy] (f32 or bf16) = x[M][ldx] (f32) * keep * scale   (N % 4 == 0): the masked
 * gradient of a dropped branch in the backward.  M >= 0 and N >= 0 (either 0 does nothing). */
int vitmi_dropout_apply(int64_t M, int64_t N, const float* x, int64_t ldx, void* y, int y_dtype,
                        int64_t ldy, uint32_t seed, uint32_t site, uint32_t thresh, float scale,
                        vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Stochastic depth / drop path (old_codes/MS_CvT.py Block.forward: x + drop_path(branch)).
 * One keep decision per SAMPLE of a drop-path site: sample b is kept iff
 * vitmi_dropout_hash(seed, path_site, b, 0) >= path_thresh (thresh = round(p * 2^32) as for
 * dropout); its factor is path_scale = 1/(1-p) if kept, else 0.  Row r of an [M, .] operand
 * belongs to sample r / rows_per_sample (the sequence length, cls token included).  Like the
 * dropout mask the factor is a pure function of its coordinates and is never stored.
 * Both calls need rows_per_sample >= 1, M % rows_per_sample == 0 and M * rows_per_sample <=
 * 2^32 (where the kernels' multiply-high row -> sample mapping is exact).  drop_thresh == 0
 * means "no element dropout" (drop_site / drop_scale are then ignored).
 *
 * vitmi_linear_fwd with the RESIDUAL epilogue (the only one accepted; dtype F32 or BF16) and
 * the sample factor fused in:
 *   y = residual + (acc + bias) * [element keep * drop_scale] * f[row / rows_per_sample]
 * (the element dropout of vitmi_linear_fwd_dropout first, then the sample factor). */
int vitmi_linear_fwd_droppath(int dtype, int64_t M, int64_t N, int64_t K, const void* x,
                              const void* w, const float* bias, void* y, int y_dtype, int epilogue,
                              const float* residual, void* workspace, size_t ws_bytes,
                              uint32_t seed, uint32_t drop_site, uint32_t drop_thresh,
                              float drop_scale, int64_t rows_per_sample, uint32_t path_site,
                              uint32_t path_thresh, float path_scale, vitmi_stream_t stream);
/* y[M][ldy] (f32 or bf16) = x[M][ldx] (f32) * f[row / rows_per_sample], with drop_thresh != 0
 * also times the element-dropout mask (keep * drop_scale) of drop_site, in the same pass: the
 * gradient entering a dropped branch in the backward.  Rows of dropped samples are zeros.
 * N % 4 == 0; alignment and leading-dimension rules of vitmi_dropout_apply. */
int vitmi_droppath_apply(int64_t M, int64_t N, const float* x, int64_t ldx, void* y, int y_dtype,
                         int64_t ldy, int64_t rows_per_sample, uint32_t seed, uint32_t path_site,
                         uint32_t path_thresh, float path_scale, uint32_t drop_site,
                         uint32_t drop_thresh, float drop_scale, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * LayerScale (CaiT; DeiT-III, BEiT, DINOv2; timm's init_values= with parameters blocks.i.ls1.gamma /
 * ls2.gamma): a learned per-channel scale gamma (fp32 [N]) on each residual branch,
 *   x + f[b] * (keep * s * (gamma o (a W^T + b)))        (a: the GEMM input; W [N][K], b [N]),
 * the element dropout keep * s and the drop-path sample factor f[b] exactly as without it.  Because
 * gamma o (a W^T + b) = a (gamma o W)^T + gamma o b, the scale is folded into the weight OPERAND of the
 * branch's last GEMM (out-projection, fc2): W_eff = gamma o W (row n of W times gamma[n]), b_eff = gamma
 * o b, and every GEMM entry point above runs unchanged on (W_eff, b_eff).  It is part of the model: the
 * same in training, evaluation and without gradients.
 *
 * Backward of one scaled linear, g the gradient entering the branch as the existing code forms it:
 *   da = g W_eff (the dgrad GEMM on the W_eff operand);  dW_eff = g^T a, db_eff = colsum(g) (the wgrad
 *   GEMM and the bias column sums, unchanged);  dW = gamma o dW_eff,  db = gamma o db_eff,
 *   dgamma[n] = sum_k dW_eff[n][k] * W[n][k] + db_eff[n] * b[n]       (W, b: the fp32 masters).
 * Nothing divides by gamma: a channel with gamma == 0 has a correct, generally nonzero dgamma.
 *
 * All four calls: fp32 masters, 16-byte accesses, no atomics, every sum in an order fixed by the shape
 * alone (bitwise reproducible).  K is a positive multiple of 8, N >= 1, N and K < 2^31 (the fold: N * K /
 * 8 < 2^31); w, w_eff, dw 16-byte aligned.  The k-major rule of the GEMM that consumes W_eff (K % 64 for
 * bf16, K % 32 for fp32) is that GEMM's to refuse.
 *
 * vitmi_layerscale_fold: w_eff[n][k] = round_to(w_dtype, fl32(gamma[n] * w[n][k])), w_dtype VITMI_F32 or
 *   VITMI_BF16: one fp32 multiply, one round-to-nearest-even.  bias_eff[n] = fl32(gamma[n] * bias[n]); bias
 *   and bias_eff are both given or both NULL.  One streaming pass (8 B or 6 B per element).
 *
 * vitmi_layerscale_bwd, in place on the gradient destinations: dw holds dW_eff and db holds db_eff.
 *   dgamma[n] += rowdot(dw[n], w[n]) + db[n] * bias[n];  then, with scale_grads = 1, dw[n][:] *= gamma[n]
 *   and db[n] *= gamma[n].  One pass over dw (each element is read once, used for the dot and written back
 *   scaled).  scale_grads = 0 leaves dw and db untouched (a frozen weight whose dW_eff lives in a
 *   temporary); dgamma NULL skips the reduction (frozen gamma; w and bias are then not read); both: no
 *   launch.  dw NULL (with dgamma NULL): only db is scaled; db NULL: a linear without bias.
 *   One wave per row for K <= 1024, one 256-thread block per row above.
 *   The call relies on dw / db holding exactly this backward's dW_eff / db_eff.  The Python layer
 *   guarantees it: a gradient destination (vitmi/grads.py GradSink) is either the parameter's ParamArena
 *   view, zeroed by begin_step at the forward and handed out once (ParamArena.take), or a buffer zeroed
 *   for this backward; the kernels of this one backward alone add into it before it is returned.  The
 *   caller orders the call after those kernels, the deferred bias-gradient folds included
 *   (vitmi_fold_end), and before the gradients leave.
 *
 * The standalone module (vitmi.LayerScale, for user-composed blocks, the counterpart of vitmi.DropPath):
 * vitmi_layerscale_apply: y[M][ldy] (f32 or bf16) = x[M][ldx] (f32) * gamma[col]: the forward, and dx from
 *   dy.  N % 4 == 0; alignment and leading-dimension rules of vitmi_dropout_apply; gamma 16-byte aligned.
 * vitmi_layerscale_dgamma: dgamma[col] += sum_m dy[m][col] * x[m][col], in two steps like vitmi_bias_grad:
 *   per-chunk partial rows in the workspace (vitmi_layerscale_dgamma_workspace_size bytes, 16-byte
 *   aligned), then the fixed-order fold (queued between vitmi_fold_begin and vitmi_fold_end).  N % 4 == 0,
 *   leading dims multiples of 4, dy and x 16-byte aligned. */
int vitmi_layerscale_fold(int64_t N, int64_t K, const float* w, const float* gamma, const float* bias,
                          void* w_eff, int w_dtype, float* bias_eff, vitmi_stream_t stream);
int vitmi_layerscale_bwd(int64_t N, int64_t K, const float* w, const float* bias, const float* gamma,
                         float* dw, float* db, float* dgamma, int scale_grads, vitmi_stream_t stream);
int vitmi_layerscale_apply(int64_t M, int64_t N, const float* x, int64_t ldx, const float* gamma, void* y,
                           int y_dtype, int64_t ldy, vitmi_stream_t stream);
size_t vitmi_layerscale_dgamma_workspace_size(int64_t M, int64_t N);
int vitmi_layerscale_dgamma(int64_t M, int64_t N, const float* dy, int64_t lddy, const float* x, int64_t ldx,
                            float* dgamma, void* workspace, size_t ws_bytes, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Patch dropout (timm's patch_drop_rate, FLIP, the MAE encoder's random masking): in training each
 * sample keeps K of its np patch tokens and the class token; every block then runs on K + 1 tokens.
 *
 * Number kept: K = max(1, int(np * (1.0 - rate))) (timm's PatchDropout), computed by the caller and
 * passed down as an integer; 1 <= K <= np <= 4096 in every call below.
 * Keys: key(b, p) = vitmi_dropout_hash(seed, PATCH_SITE, row = b, col = p), PATCH_SITE = 0x20000000
 * (disjoint from the dropout sites 3i..3i+2 and from the drop-path sites 0x40000000 + ...); seed is
 * the forward's single drop seed.
 * Which patches are kept: sample b keeps the K patches with the smallest (key, p) pairs, in
 * lexicographic order (ties are broken by the smaller p).  Two index tensors describe the subset:
 *   keep[b][0..K) (int32): the kept patch numbers in ASCENDING order;
 *   slot[b][p]    (int32): the position j of patch p in keep[b], or -1 when dropped.
 * Token tensor: [B, K + 1, D]; row 0 is cls + pos[0], row 1 + j is tok(b, keep[b][j]) +
 * pos[1 + keep[b][j]].  Nothing is rescaled; everything downstream sees a model with N = K + 1.
 * Backward: dcls and dpos[0] as in vitmi_tokens_assemble_bwd; dpos[1 + p] += sum_b dx[b][1 +
 * slot[b][p]] over the samples that kept p, b in ascending order by one thread per (p, d), no
 * atomics: bitwise reproducible.  dW, dbias of the patch projection come from the B*K kept rows.
 * The gathered kernels treat an index outside [0, np) as "no patch": the forward writes a zero
 * row, the backward adds nothing.
 *
 * vitmi_patch_keep: one block per sample builds keep [B][K] and slot [B][np] (np^2 compares per
 * sample on keys held in LDS); a pure function of (seed, site, b), no host read. */
int vitmi_patch_keep(int B, int np, int K, uint32_t seed, uint32_t site, int32_t* keep, int32_t* slot,
                     vitmi_stream_t stream);
/* vitmi_patch_im2col with row b*K + j reading patch keep[b][j]: patches [B*K][C*P*P] of dtype */
int vitmi_patch_im2col_keep(int dtype, int B, int C, int S, int P, int K, const int32_t* keep,
                            const float* img, void* patches, vitmi_stream_t stream);
/* x[b][0] = cls + pos[0];  x[b][1+j] = tok[b*K+j] + pos[1 + keep[b][j]]   (cls/pos may be NULL) */
int vitmi_tokens_assemble_keep(int B, int np, int K, int D, const float* tok, const float* cls,
                               const float* pos, const int32_t* keep, float* x, vitmi_stream_t stream);
/* backward of the gathered assemble: dtok [B*K][D] (f32, and/or a bf16 copy) = dx[:,1:];  dpos
 * [np+1][D] and dcls += the sums above   (NULL pointers skip that output) */
int vitmi_tokens_assemble_keep_bwd(int B, int np, int K, int D, const float* dx, float* dtok,
                                   void* dtok_lp, float* dcls, float* dpos, const int32_t* slot,
                                   vitmi_stream_t stream);
/* vitmi_patch_embed_fwd / _bwd over the kept patches: the same composition from the gathered pieces
 * (bit-identical to calling them), the patch GEMM and its gradients at M = B*K rows.
 * patches: [B*K][C*P*P] of dtype; x and dx: fp32 [B][K+1][D]; dpos: [np+1][D]. */
size_t vitmi_patch_embed_keep_fwd_workspace_size(int dtype, int B, int C, int S, int P, int D, int K);
int vitmi_patch_embed_keep_fwd(int dtype, int B, int C, int S, int P, int D, int K, const int32_t* keep,
                               const float* img, const void* w, const float* bias, const float* cls,
                               const float* pos, void* patches, float* x, void* workspace, size_t ws_bytes,
                               vitmi_stream_t stream);
size_t vitmi_patch_embed_keep_bwd_workspace_size(int dtype, int B, int C, int S, int P, int D, int K);
int vitmi_patch_embed_keep_bwd(int dtype, int B, int C, int S, int P, int D, int K, const int32_t* slot,
                               const float* dx, const void* patches, float* dw, float* dbias, float* dcls,
                               float* dpos, void* workspace, size_t ws_bytes, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * CvT stages (the reference's actual SLS model, models/CvT(Par).py:66-72).
 *
 * ConvEmbed = layers.Conv2D(D, kernel=k, strides=s, padding='same') (:203-212) as a GEMM over
 * patches.  TF 'same': Ho = ceil(H/s), pad_total = max((Ho-1)s + k - H, 0), pad_before =
 * pad_total/2 (vitmi_conv_same_geometry).  Input rows are NHWC tokens: image b, pixel (h, w)
 * is row b*img_stride + row_off + h*W + w of x [..][ldx] (fp32).  Patch rows [B*Ho*Wo][Kp]
 * (dtype) in column order (kh, kw, c) -- the Keras kernel [kh][kw][Cin][Cout] flattened --
 * zero-padded to Kp (a multiple of the GEMM's K step).
 */
int vitmi_conv_same_geometry(int H, int W, int kh, int kw, int s, int* Ho, int* Wo, int* pad_top, int* pad_left);
/* explicit geometry (pad_top/pad_left/Ho/Wo): TF 'same' from vitmi_conv_same_geometry, or the
 * symmetric padding of torch Conv2d (old_codes/MS_CvT.py PATCH_PADDING) */
int vitmi_conv_im2col(int dtype, int B, int H, int W, int C, int kh, int kw, int s, int pad_top, int pad_left,
                      int Ho, int Wo, const float* x, int64_t ldx, int64_t img_stride, int64_t row_off,
                      void* patches, int Kp, vitmi_stream_t stream);
/* adjoint of im2col: dx (f32, rows as x) (+)= the sum over every window reading a pixel (C % 4 == 0) */
int vitmi_conv_col2im(int dtype, int B, int H, int W, int C, int kh, int kw, int s, int pad_top, int pad_left,
                      int Ho, int Wo, const void* dpatches, int Kp, float* dx, int64_t ldx, int64_t img_stride,
                      int64_t row_off, int accumulate, vitmi_stream_t stream);
/* Projection(method='dw_bn') (:83-112): z = DepthwiseConv2D(3, 'same', no bias)(x) [3][3][C],
 * y = BatchNormalization: training != 0 -> batch statistics over n = B*H*W (biased variance) and the
 * moving statistics m <- momentum m + (1-momentum) stat (NULL to skip; the moving variance takes
 * the unbiased n/(n-1) estimate, as Keras' fused BN and torch's BatchNorm2d do); training == 0 -> the
 * moving statistics normalise (Keras inference).  x/dx rows as above (cls row skipped via
 * x_off), y rows b*y_img + y_off + hw of y [..][ldy] (y_dtype).  z [B*H*W][C], mean/rstd [C]
 * are saved for the backward.  C % 4 == 0 and 1024 % C == 0.  Every pitch is a multiple of 4 and >= C,
 * every offset >= 0, y_dtype / dy_dtype VITMI_F32 or VITMI_BF16; the fp32 pointers the kernels read or
 * write four channels at a time (x, w, gamma, beta, z, mean, rstd, dx, the workspace; dx of
 * vitmi_conv_col2im and of vitmi_avgpool3_bwd, x of vitmi_avgpool3_fwd) must be 16-byte aligned. */
size_t vitmi_dwconv_bn_workspace_size(int B, int H, int W, int C);
int vitmi_dwconv_bn_fwd(int B, int H, int W, int C, const float* x, int64_t ldx, int64_t x_img, int64_t x_off,
                        const float* w, const float* gamma, const float* beta, float eps, float momentum,
                        int training, float* run_mean, float* run_var, float* z, float* mean, float* rstd, void* y,
                        int y_dtype,
                        int64_t ldy, int64_t y_img, int64_t y_off, void* workspace, size_t ws_bytes,
                        vitmi_stream_t stream);
/* dx += d/dx, dw/dgamma/dbeta += (f32) from dy (rows as y, dy_dtype) */
int vitmi_dwconv_bn_bwd(int B, int H, int W, int C, const void* dy, int dy_dtype, int64_t lddy, int64_t dy_img,
                        int64_t dy_off, const float* x, int64_t ldx, int64_t x_img, int64_t x_off, const float* w,
                        const float* gamma, const float* z, const float* mean, const float* rstd, float* dx,
                        float* dw, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                        vitmi_stream_t stream);

/* Projection(method='avg') (models/CvT(Par).py:95-96,107-108): AveragePooling2D(pool 3,
 * stride 1, padding 'same') over [B, H, W, C] token rows laid out like vitmi_dwconv_bn_fwd's
 * (image b pixel p at row b*x_img + x_off + p), the mean over the in-bounds taps (TF 'same'
 * pooling excludes the padding from the divisor; count_pad=1: always 9, torch's AvgPool2d as in
 * old_codes/MS_CvT.py:145-153).  y (bf16 | f32) rows likewise.  The
 * backward ACCUMULATES dx += pool^T(dy).  C % 4 == 0, 1024 % C == 0. */
int vitmi_avgpool3_fwd(int B, int H, int W, int C, const float* x, int64_t ldx, int64_t x_img, int64_t x_off,
                       void* y, int y_dtype, int64_t ldy, int64_t y_img, int64_t y_off, int count_pad,
                       vitmi_stream_t stream);
int vitmi_avgpool3_bwd(int B, int H, int W, int C, const void* dy, int dy_dtype, int64_t lddy, int64_t dy_img,
                       int64_t dy_off, float* dx, int64_t ldx, int64_t x_img, int64_t x_off, int count_pad,
                       vitmi_stream_t stream);

/* Small fp32 Dense layers: Proc_Dense_1/2 = layers.Dense(256, activation='relu') on the
 * standardised process parameters (models/CvT(Par).py:343-344).  y = act(x W^T + b),
 * act 0 = linear, 1 = relu; x [M][ldx], W [N][K] fp32, y [M][ldy].  The backward takes the
 * forward's output y (the relu mask), writes dx = (dy * act'(y)) W when dx != NULL and
 * ACCUMULATES dW += (dy * act'(y))^T x, db += column sums (db may be NULL).  Exact fp32 FMA
 * in a fixed order (deterministic). */
int vitmi_dense_f32_fwd(int M, int N, int K, const float* x, int64_t ldx, const float* w, const float* b, float* y,
                        int64_t ldy, int act, vitmi_stream_t stream);
int vitmi_dense_f32_bwd(int M, int N, int K, const float* dy, int64_t lddy, const float* y, int64_t ldy,
                        const float* x, int64_t ldx, const float* w, float* dx, int64_t lddx, float* dw, float* db,
                        int act, vitmi_stream_t stream);

/* Keras Adam step (models/CvT(Par).py:458-460: keras.optimizers.Adam(1e-3); beta_1 0.9,
 * beta_2 0.999, epsilon 1e-7) over n fp32 parameters in place:
 *   g' = g * grad_scale;  m += (g' - m)(1 - b1);  v += (g'^2 - v)(1 - b2);
 *   p -= alpha m / (sqrt(v) + eps),   alpha = lr sqrt(1 - b2^t) / (1 - b1^t) (caller, step t >= 1).
 * p_lp (optional, bf16) receives the updated parameters' operand shadow in the same pass.
 * (1 - beta) is formed in double and rounded once (Keras' Python-float hyper-parameters).
 * Explicitly rounded fp32 ops in this order: bit-identical to a float32 evaluation.  Buffers
 * 16-byte aligned (a ParamArena's flat buffers; one launch for the whole model). */
int vitmi_adam_step(int64_t n, float* p, const float* g, float* m, float* v, void* p_lp, float alpha, double beta_1,
                    double beta_2, float epsilon, float grad_scale, vitmi_stream_t stream);

/* Global-norm clipping, decoupled weight decay and non-finite step skipping for the Adam step
 * (keras.optimizers.Adam(global_clipnorm=, weight_decay=)), decided on the device: no host read.
 *
 * vitmi_grad_sumsq: partials[c] = sum of (double)g[i]^2 over chunk c = [c CHUNK, min(n, (c+1) CHUNK)),
 *   CHUNK = VITMI_GRAD_SUMSQ_CHUNK elements; vitmi_grad_sumsq_partials(n) = ceil(n / CHUNK) doubles.
 *   Each element is widened to fp64 before squaring (exact), every addition is fp64, in an order
 *   fixed by the chunk alone (per thread, wave64 cross-lane, one fold through LDS; no atomics): a
 *   partial does not depend on n, the grid or the device, so results are bitwise reproducible.
 *   One streaming read of g (16-B loads; g 16-byte aligned, any n), one block per chunk.
 *   CHUNK = 8192 (32 KiB of loads in flight per block; see DESIGN.md for the measurement).
 * vitmi_clip_finalize: one block folds partials[0 .. n_partials) (thread t takes t, t + 256, ...
 *   in ascending order, then the same fixed tree) and writes the 16-byte device record
 *     struct { float coef; float norm; uint32_t skip; uint32_t skipped_total; }
 *   norm = (float)(|grad_scale| sqrt(total));  coef = norm > clip_norm ? clip_norm / norm : 1.0f
 *   (one fp32 division; exactly 1 when nothing is clipped; clip_norm == 0: off, coef = 1);
 *   skip = skip_nonfinite && !isfinite(total);  skipped_total += skip.  A non-finite total gives
 *   coef = NaN: without skip_nonfinite the NaN reaches every parameter, as in Keras.  The caller
 *   zeroes the record once.  partials 8-byte, ctl 16-byte aligned; clip_norm >= 0.
 * vitmi_adam_step_ctl: vitmi_adam_step (same rounded fp32 ops, same order) with
 *   g' = (g * grad_scale) * coef        (the second product only if coef != 1; coef from ctl)
 *   p  = p - (p * weight_decay) * lr    before the update, if weight_decay != 0 and the element's
 *        64-element group has its byte of decay_mask set (ceil(n / 64) bytes; NULL: every group)
 *   and, if ctl->skip, p, m and v left bit for bit as they were (p_lp is still written as
 *   bf16(p)).  ctl == NULL: coef 1, never skipped.  With ctl == NULL and weight_decay == 0 the
 *   results equal vitmi_adam_step's bitwise.  weight_decay >= 0; ctl 16-byte aligned. */
#ifndef VITMI_GRAD_SUMSQ_CHUNK
#define VITMI_GRAD_SUMSQ_CHUNK 8192
#endif
size_t vitmi_grad_sumsq_partials(int64_t n);
int vitmi_grad_sumsq(int64_t n, const float* g, double* partials, vitmi_stream_t stream);
int vitmi_clip_finalize(int64_t n_partials, const double* partials, float grad_scale, float clip_norm,
                        int skip_nonfinite, void* ctl, vitmi_stream_t stream);
int vitmi_adam_step_ctl(int64_t n, float* p, const float* g, float* m, float* v, void* p_lp, float alpha,
                        double beta_1, double beta_2, float epsilon, float grad_scale, float weight_decay, float lr,
                        const uint8_t* decay_mask, const void* ctl, vitmi_stream_t stream);

/* Exponential moving average of the weights (keras.optimizers.Adam(use_ema=True, ema_momentum=)),
 * kept inside the step, and its use for evaluation.
 *
 * vitmi_adam_step_ema: vitmi_adam_step_ctl (same arguments, same meaning, same rounded fp32 ops in
 *   the same order; ctl == NULL, weight_decay == 0 and decay_mask == NULL allowed, so it covers the
 *   plain, decayed and clipped steps) followed, per element, by
 *     e = (mom * e) + (one_m * p_new)     (two products and one sum, each rounded; no FMA)
 *   with mom = ema_momentum and one_m = 1.0f - mom formed once on the host in fp32 (Keras forms
 *   1 - momentum in the variable's dtype).  mom == 0 runs the same three ops.  If ctl->skip, ema
 *   is neither read nor written: p, m, v and ema stay bit for bit, p_lp is still written as
 *   bf16(p).  ema: fp32, 16-byte aligned, required; ema_momentum in [0, 1).  4 B read and 4 B
 *   written per parameter on top of the step's (38 B with the shadow, 36 B without).
 * vitmi_ema_apply: mode 0 exchanges p and ema in place (no temporary); mode 1 writes p <- ema and
 *   leaves ema as it is.  p_lp (optional, bf16) receives the shadow of the new p in the same pass.
 *   p and ema fp32, 16-byte aligned; p_lp 8-byte aligned; any n >= 0. */
int vitmi_adam_step_ema(int64_t n, float* p, const float* g, float* m, float* v, void* p_lp, float alpha,
                        double beta_1, double beta_2, float epsilon, float grad_scale, float weight_decay, float lr,
                        const uint8_t* decay_mask, const void* ctl, float* ema, float ema_momentum,
                        vitmi_stream_t stream);
int vitmi_ema_apply(int64_t n, float* p, float* ema, void* p_lp, int mode, vitmi_stream_t stream);

/* The classification recipe on the device (csrc/loss.hip): softmax cross-entropy on label, mixed-pair
 * and dense soft targets with label smoothing and top-1 / top-k scoring, and the mixup / cutmix image
 * pass (timm Mixup + SoftTargetCrossEntropy; tf.keras CategoricalCrossentropy(label_smoothing=)).
 *
 * vitmi_softmax_xent: logits fp32 [B][ldl], C classes.  The target distribution of row b is
 *   label form (soft == NULL):  t = lam[b] onehot(label_a[b]) + (1 - lam[b]) onehot(label_b[b]);
 *     label_b and lam are both NULL (t = onehot(label_a[b])) or both given;
 *   dense form (soft fp32 [B][lds]):  t = soft[b][:], which need not sum to 1;
 *   q = (1 - smoothing) t + smoothing sum(t) / C    (smoothing == 0: q = t exactly).
 *   row_loss[b]   = lse_b sum(q) - sum_c q_c z_c    (a class with q_c == 0 adds nothing, even at
 *                   z_c = -inf: masked classes give a finite loss and a zero gradient there)
 *   dlogits[b][c] = (softmax(z)_c sum(q) - q_c) / B,  softmax as exp(z - max) / sum;  [B][lddl],
 *                   columns past C are not written
 *   loss[0]       = (float)(sum_b (double)row_loss[b] / B)
 *   Label values are not read on the host.  A label outside [0, C) matches no class: it keeps its
 *   weight in sum(t) but has no indexed logit and no gradient entry (row_loss = lse sum(q) minus the
 *   smoothing term alone), and the row is a miss.
 *   Non-finite logits: nothing is hidden.  A row that holds a NaN logit, at any column and on either
 *   load path, has row_loss[b] = NaN and every dlogits[b][c] = NaN, and loss[0] (and loss_sum) is NaN;
 *   the other rows of the batch keep their bits.
 *   One wave64 per row, one online (max, sum) pass with 16-byte loads when C % 4 == 0, ldl (lds, lddl)
 *   % 4 == 0 and the bases are 16-byte aligned, scalar loads otherwise; the gradient leaves from
 *   registers for C <= 1024 and from a second (L2) pass above.  A row's results depend on that row
 *   alone; a second launch of one block folds the rows in fp64 (thread t takes rows t, t + 256, ... in
 *   ascending order, then a fixed tree, as vitmi_clip_finalize): results are bitwise reproducible.
 *   row_loss, loss and dlogits may each be NULL, but not all three without metrics.
 * metrics (optional): a 32-byte, 16-byte aligned device record the caller zeroes once,
 *     struct { double loss_sum; uint64_t rows; uint64_t top1; uint64_t topk; }
 *   The fold launch ADDS this batch: loss_sum += sum_b row_loss[b], rows += B, and the hit counts; the
 *   host reads it once per epoch.  Hits are scored against y = label_a[b] (required with metrics, in the
 *   dense form too), on the fp32 logits exactly: row b is a top-k hit iff
 *     #{c : z_c > z_y or (z_c == z_y and c < y)} < k        (ties go to the lower class index)
 *   top-1 is the same rule with k = 1; a row whose z_y is NaN, or whose label is outside [0, C), is a
 *   miss.  topk in 0..C, >= 1 with metrics.
 * workspace: vitmi_softmax_xent_workspace_size(B) bytes (row losses when row_loss is NULL, one flag
 *   byte per row); required with metrics, or with loss when row_loss is NULL; 4-byte aligned.
 *   B > 0, 1 <= C <= 65535, ldl / lds / lddl >= C, 0 <= smoothing < 1.
 *
 * vitmi_mix_batch: mixup and cutmix of an fp32 [B][C][H][W] batch in one pass,
 *   out[b,c,y,x] = (y0 <= y < y1 && x0 <= x < x1) ? img[perm[b],c,y,x]
 *                                                 : lam[b] img[b,c,y,x] + (1 - lam[b]) img[perm[b],c,y,x]
 *   with the per-sample device tables perm int32 [B], lam fp32 [B], box int32 [B][4] = (y0, y1, x0, x1).
 *   An empty box gives pure mixup, lam = 1 with a box pure cutmix.  1 - lam is formed once in fp32, the
 *   two products are rounded separately and then added (no FMA): bit-identical to a float32 evaluation.
 *   A sample with lam == 1 and an empty box is a copy whose partner is not read (a NaN there cannot leak
 *   through 0 * NaN).  Box edges are clamped to the image and perm[b] outside [0, B) is taken as b, in
 *   the kernel.  16-byte accesses along x when W % 4 == 0 and img, out are 16-byte aligned (selected per
 *   element inside a group that straddles a box edge), scalar otherwise.  out must not overlap img. */
size_t vitmi_softmax_xent_workspace_size(int B);
int vitmi_softmax_xent(int B, int C, const float* logits, int64_t ldl, const int64_t* label_a, const int64_t* label_b,
                       const float* lam, const float* soft, int64_t lds, float smoothing, int topk, float* row_loss,
                       float* loss, float* dlogits, int64_t lddl, void* metrics, void* workspace,
                       size_t workspace_bytes, vitmi_stream_t stream);
int vitmi_mix_batch(int B, int C, int H, int W, const float* img, const int* perm, const float* lam, const int* box,
                    float* out, vitmi_stream_t stream);

/* SLS data pipeline (models/CvT(Par).py:414-428).
 * vitmi_sls_resize_table (host): cv2 INTER_LINEAR table of one axis, ssize -> dsize:
 *   ofs[d] first source index, w[2d], w[2d+1] its Q11 weights (OpenCV 8-bit fixed point).
 * vitmi_sls_preprocess: n decoded uint8 frames (interleaved 3 channels, RGB, or BGR if bgr=1;
 *   frame i row y at src + i*img_bytes + y*row_bytes) -> cv2.resize to Wo x Ho ->
 *   BGR2GRAY -> /255.0 -> fp32 out[n][Ho*Wo].  Tables are device copies of the two axis
 *   tables (xofs/xw for W -> Wo, yofs/yw for H -> Ho).
 * vitmi_gather_rows: dst[i] = src[idx[i]] for n rows of row_bytes (batch assembly from the
 *   HBM-resident dataset; idx device int64; an index outside [0, n_src) gives a zero row). */
int vitmi_sls_resize_table(int ssize, int dsize, int* ofs, short* w);
int vitmi_sls_preprocess(int n, int H, int W, const void* src, int64_t img_bytes, int64_t row_bytes, int bgr, int Ho,
                         int Wo, const int* xofs, const short* xw, const int* yofs, const short* yw, float* out,
                         vitmi_stream_t stream);
int vitmi_gather_rows(int64_t n, int64_t row_bytes, const void* src, int64_t n_src, const int64_t* idx, void* dst,
                      vitmi_stream_t stream);

/* Split-bf16 operands of the precision knob (ViTConfig dtype "bf16x3"; csrc/split.hip).  The reference
 * computes in fp32 (models/CvT(Par).py, Keras floatx); an operand carried as x = hi + lo, hi = bf16(x),
 * lo = bf16(x - hi), makes a bf16 MFMA product good to ~2^-16: hi.hi + hi.lo + lo.hi, computed by the
 * GEMMs above unchanged as ONE product over K' = 3K with the A rows laid out [hi | hi | lo] (pattern 0)
 * and the weight rows [hi | lo | hi] (pattern 1).
 *   vitmi_split_bf16x3: src fp32 [rows][ld_src] (K % 4 == 0) -> dst bf16 [rows][ld_dst >= 3K];
 *     hi_copy (optional, bf16 [rows][ld_copy]) receives hi alone (the bf16 operand of the backward).
 * The activation operands come split straight from their producers: vitmi_layernorm_fwd (y dtype
 * VITMI_BF16X3), vitmi_attention_fwd_x3 and the fc1 epilogue (VITMI_EPI_SPLIT_X3). */
int vitmi_split_bf16x3(int64_t rows, int64_t K, const float* src, int64_t ld_src, void* dst, int64_t ld_dst,
                       int pattern, void* hi_copy, int64_t ld_copy, vitmi_stream_t stream);
/* VITMI_BF16F8 rows: src fp32 [rows][ld_src] (K % 64 == 0) -> dst [rows][ld_dst >= 2K bf16 units],
 * pattern 0 the A-operand layout (e4m3 blocks [hi8 | lo8]), pattern 1 the weight layout ([lo8 | hi8]);
 * patterns 2 / 3: the VITMI_BF16F8W rows (ld_dst >= 1.5K bf16 units, K % 128 == 0), [hi | hi8] (A
 * operand) / [hi | lo8] (weight); hi_copy as above. */
int vitmi_split_bf16f8(int64_t rows, int64_t K, const float* src, int64_t ld_src, void* dst, int64_t ld_dst,
                       int pattern, void* hi_copy, int64_t ld_copy, vitmi_stream_t stream);
/* Up to 8 dense weights (srcs[j] fp32 [rows[j]][K[j]]) to pattern-1 VITMI_BF16F8 rows (dsts[j]
 * [rows[j]][2 K[j]] bf16 units) in one launch (the knob's per-forward weight split). */
int vitmi_split_bf16f8_weights(int n, const float* const* srcs, void* const* dsts, const int64_t* rows,
                               const int64_t* K, vitmi_stream_t stream);
/* The same with a layout per weight: patterns[j] 1 (VITMI_BF16F8 rows, [rows][2K]) or 3
 * (VITMI_BF16F8W rows [hi | lo8], [rows][1.5K], K % 128 == 0: the qkv weight of the bf16f8 knob). */
int vitmi_split_bf16f8_weights_mixed(int n, const float* const* srcs, void* const* dsts, const int64_t* rows,
                                     const int64_t* K, const int* patterns, vitmi_stream_t stream);

/* fp32 -> bf16 cast of n >= 0 elements (weight shadows for the bf16 MFMA path); src and dst 16-byte aligned */
int vitmi_cast_f32_bf16(int64_t n, const float* src, void* dst, vitmi_stream_t stream);
/* bf16 -> fp32 cast of n >= 0 elements (the bf16 gradient all-reduce writes back into the fp32 arena);
 * src and dst 16-byte aligned */
int vitmi_cast_bf16_f32(int64_t n, const void* src, float* dst, vitmi_stream_t stream);

/* ---------------------------------------------------------------------------
 * Data-parallel gradient exchange over RCCL (xGMI within a node).  Replaces the cross-replica
 * gradient reduction of tf.distribute.MirroredStrategy (old_codes/BayConvT(Par)(Muti).py:16-19,
 * the reference's only parallel construct; TF runs it as an NCCL all-reduce on one host).
 * One process per GPU, one communicator per process (bound to the HIP device current at
 * vitmi_comm_init).  Rank 0 creates the 128-byte id; the caller distributes it (vitmi/dp.py
 * uses torch.distributed's TCPStore).  RCCL is bound at run time (the copy already loaded by
 * the process, else librccl.so); errors return VITMI_ERR_COMM.
 */
#define VITMI_COMM_UID_BYTES 128
enum { VITMI_REDUCE_SUM = 0, VITMI_REDUCE_AVG = 1 };
int vitmi_comm_get_unique_id(char* uid /* [VITMI_COMM_UID_BYTES] */);
int vitmi_comm_init(int rank, int world, const char* uid /* [VITMI_COMM_UID_BYTES] */);
int vitmi_comm_info(int* rank, int* world);
/* file name of the RCCL library the comm leg bound (dladdr of its ncclAllReduce): the copy
 * torch already mapped, so the process holds one RCCL instance */
int vitmi_comm_library(char* path, int len);
/* In-place all-reduce of `count` elements (VITMI_F32 | VITMI_BF16 | VITMI_F64) on the side stream `side`,
 * after `ready_event` (a hipEvent_t recorded on the compute stream, may be NULL).  Returns once
 * enqueued; the caller orders its consumers after `side` (record an event / stream wait). */
int vitmi_comm_allreduce_async(void* ptr, int64_t count, int dtype, int op, vitmi_stream_t side, void* ready_event);
/* in-place broadcast from `root` (parameter replication at start-up) */
int vitmi_comm_broadcast(void* ptr, int64_t count, int dtype, int root, vitmi_stream_t stream);
/* VITMI_ERR_COMM if the communicator reported an asynchronous error */
int vitmi_comm_check(void);
/* abort != 0: ncclCommAbort (tear down after a peer failure without waiting) */
int vitmi_comm_destroy(int abort);

/* Deferred partial-sum folds.  The parameter-gradient outputs of vitmi_layernorm_bwd (dgamma, dbeta,
 * dxsum), of the fused column sums of vitmi_linear_dgrad_bias / vitmi_attention_bwd_bias and of
 * vitmi_bias_grad are formed in two steps: per-block partial rows in the caller's workspace, then a
 * small fold launch (out += the column sums of the partial rows, fixed order).  Between
 * vitmi_fold_begin() and vitmi_fold_end() on one host thread, those folds are queued instead of
 * launched, and vitmi_fold_end launches them together (one launch per 16 folds, on the stream of the
 * calls that queued them) and orders `stream` after every other stream that ran folds since
 * vitmi_fold_begin (an event wait).  The caller keeps the workspaces of the queued calls alive until
 * then; the outputs are final in `stream` order after vitmi_fold_end.  vitmi/modules.py brackets
 * each block's backward with them: one fold launch per block instead of four. */
int vitmi_fold_begin(void);
int vitmi_fold_end(vitmi_stream_t stream);

/* Compute units the persistent GEMM leaves free (default 0): with data-parallel gradient
 * all-reduces in flight, RCCL's kernels need CUs while a one-block-per-CU GEMM would hold all
 * of them for its whole duration.  Returns the previous value. */
int vitmi_gemm_set_reserved_cus(int n);

#ifdef __cplusplus
}
#endif
#endif /* VITMI_H */
