/*
 * dfx_gemm_bf16.h -- C ABI of the bf16 MFMA GEMM (gfx950, v_mfma_f32_32x32x16_bf16, fp32 accumulation) behind the opt-in
 * bf16 FFNs of the inference path (csrc/gemm_bf16.hip; dfx.ops.linear_bf16; models.fused.LINEAR_BF16).
 *
 *   C[M,N] = act(A[M,K] x W[N,K]^T + bias[N] (+ R[M,N]))
 *
 * Dtype codes: DFX_DT_F32 = 0, DFX_DT_BF16 = 1, for A (a_dtype) and for C (c_dtype) independently; all four combinations.
 * W is bf16 [N,K] (an nn.Linear weight, converted once by the caller), bias and the residual R are fp32 or NULL.
 *
 * Arithmetic.  An fp32 A is rounded to bf16 with round-to-nearest-even while it is staged - the rounding of
 * tensor.to(torch.bfloat16) - and no bf16 copy of it is written to memory.  Products are exact in fp32 and are accumulated in
 * fp32 in ascending k, one chain per output element (no split-K, no atomics: two calls give the same bits).  Bias, residual and
 * the activation (DFX_ACT_*: 0 none, 1 ReLU, 2 exact GELU) are fp32; a bf16 C is rounded once, from that fp32 value.
 *
 * Shapes.  K a multiple of 8; rows of A and W 16-byte aligned (A, W and lda * sizeof(element), ldw * 2); any M >= 1 and N >= 1.
 * Row pitches in elements, lda >= K, ldw >= K, ldr >= N, ldc >= N.  C leaves in 16-byte stores when N is a multiple of 8 and the
 * rows of C (and of R) are 16-byte aligned, element by element otherwise (C, bias and R aligned to their element size: an odd N
 * with a bf16 C means 2-byte aligned rows).  Nothing outside [M, N] of C is written.
 *
 * Device pointers, enqueue-only on `stream`.  DFX_EINVAL for null pointers, bad dimensions, K % 8, pitches shorter than the row,
 * misalignment, an activation outside 0 .. 2 or an unknown dtype code; DFX_ERANGE when an operand of the call (A, W, R or C)
 * reaches 2 GiB - all before any launch, with a dfx_last_error() text.  M * N == 0 returns DFX_OK without a launch.
 * An addition to the ABI: dfx_abi_version() stays.
 */
#ifndef DFX_GEMM_BF16_H
#define DFX_GEMM_BF16_H

#include "dfx_conv.h" /* DFX_ACT_* */

#define DFX_DT_F32 0
#define DFX_DT_BF16 1

#ifdef __cplusplus
extern "C" {
#endif

int dfx_gemm_bf16(const void *A, int a_dtype, long lda,
                  const void *W, long ldw,
                  const float *bias,
                  const float *R, long ldr,
                  void *C, int c_dtype, long ldc,
                  int M, int N, int K, int act, void *stream);

/*
 * The weight gradient of a Linear that trains on bf16 products (csrc/gemm_bf16_wgrad.hip; dfx.ops.linear_bf16_backward;
 * models.fused.LINEAR_BF16_TRAIN):
 *
 *   dW[n][k] = sum_m bf16(dY[m][n]) * bf16(X[m][k])      [N, K] fp32, row pitch ldw
 *   db[n]    = sum_m dY[m][n]                            [N] fp32, from the UNROUNDED fp32 values; NULL: not computed
 *
 * dY [M,N] and X [M,K] are fp32, row-major, row pitches ldy and ldx in elements.  Both are rounded to bf16 (round-to-nearest-even)
 * while they are staged; no bf16 copy of either is written to memory.  Products are exact, accumulation is fp32.
 *
 * M is cut into `splits` ranges of whole 32-row steps (clamped so that no range is empty), exactly as dfx_gemm_wgrad_f32
 * (dfx_gemm.h) cuts it into 16-row steps.  Each range writes a partial slab to the caller-owned `workspace` of
 * splits * (N*K + N) floats and one reduction launch adds the slabs in ascending range order: no atomics, two calls give the
 * same bits.  One range stores directly, and `workspace` may then be NULL.  Outputs are overwritten, never accumulated into.
 *
 * DFX_EINVAL for negative dimensions or splits < 1, null pointers, N or K not multiples of 8, ldy / ldx / ldw not multiples of 4
 * or shorter than the row, dY / X / dW / workspace not 16-byte aligned, more than one range without a workspace; DFX_ERANGE
 * when dW, or one range of dY or X, reaches 2 GiB - all before any launch, with a dfx_last_error() text.  N*K == 0 returns
 * DFX_OK without a launch; M == 0 writes zeros.  An addition to the ABI: dfx_abi_version() stays.
 */
int dfx_gemm_bf16_wgrad(const float *dY, long ldy, const float *X, long ldx, float *dW, long ldw,
                        float *db, int M, int N, int K, int splits, float *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_GEMM_BF16_H */
