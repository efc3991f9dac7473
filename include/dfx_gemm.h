/*
 * dfx_gemm.h -- C ABI of the hand-written fp32 MFMA GEMM (gfx950, v_mfma_f32_32x32x2_f32) with the
 * fused prologue / epilogues the deformable-attention path needs.
 *
 * It stands where the reference calls PyTorch library GEMMs on this path:
 *   nn.Linear value_proj / sampling_offsets / attention_weights / output_proj
 *                                   /root/reference/models/ops/modules/ms_deform_attn.py:94-100,116
 *   FFN linear1 (+ReLU) / linear2   /root/reference/models/deformable_transformer_single.py:544-548
 *   Late Fusion adapt / FFN Linears /root/reference/models/deformable_transformer_single.py:379-402
 *   1x1 convolutions of ResNet-50 (+ folded FrozenBatchNorm2d, ReLU, residual add)
 *                                   /root/reference/models/backbone_scratch.py:102-141 (torchvision Bottleneck)
 *   input_proj 1x1 convolution      /root/reference/models/deformable_detr_single.py:101-125
 *
 *   C[b] = act( (A[b] (+ A2[b])) x op(B[b]) + bias (+ R[b]) ), rows with row_mask != 0 forced to 0
 *
 *   A   [M,K] row-major, leading dimension lda; batch stride strideA (0 = shared by all batches)
 *       or, with a_block_stride > 0, K-block-major [K/4][M][4]: element (m, k) at
 *       A[(k / 4) * a_block_stride + m * 4 + k % 4] (the layout the level-in-LDS MSDA kernel writes its
 *       output in, consumed by output_proj; lda is ignored, no A2)
 *   A2  optional, same layout as A, added element-wise while A is staged (query = src + pos)
 *   B   b_is_kn = 1: [K,N] row-major (ldb >= N)  -- activations of a 1x1 convolution, NCHW
 *       b_is_kn = 0: [N,K] row-major (ldb >= K)  -- an nn.Linear weight
 *   bias optional; bias_per_row = 1: bias[m] (convolution), 0: bias[n] (Linear)
 *   R   optional residual, layout of C (ldr, strideR)
 *   row_mask optional uint8[M] per batch (strideMask): value_proj's masked_fill of padded tokens
 *   C   [M,N] row-major, ldc; or, with c_block = w > 0, column-block-major: element (m, n) at
 *       C[(n / w) * c_block_stride + m * w + n % w] - the layout the level-in-LDS MSDA kernel
 *       (dfx_msda.h) reads: value_proj output as [32 channel octets][tokens][8], the joint
 *       sampling_offsets / attention_weights output as [8 heads][queries][12] (no residual then).
 *       A wide block (w a multiple of 128, [N,K] operand) stacks Linears that share A: every block is
 *       a contiguous [M, w] result of its own (the value projections of the six decoder layers over one
 *       memory, /root/reference/models/deformable_transformer_single.py:703-748); they run as one launch
 *       that reads an A panel once for the whole stack
 *   relu 0: none, 1: ReLU, 2: exact (erf) GELU (nn.GELU() of the fusion blocks' FFN,
 *       /root/reference/models/deformable_transformer_single.py:379-402)
 * fp32 in, fp32 accumulate (exact fp32 MFMA), fp32 out.  K must be a multiple of 4; A, B rows
 * 16-byte aligned.  Same conventions as dfx_msda.h (device pointers, enqueue-only, 0 / <0).
 *
 * dfx_gemm_splitk_f32: the same product for problems with few output tiles and a long K (RCNNHead's
 * out_layer 12544 -> 256 over 300 rows per frame, /root/reference/models/sparse_roi_head/head.py:127-172):
 * K is cut into ``splits`` ranges of whole 16-deep steps that run as independent workgroups writing partial
 * [M,N] slabs to ``workspace`` (splits * M * N floats, caller-owned), followed by one reduction launch that
 * adds the slabs, bias, residual and applies the activation.  Row-major A [M,K], C [M,N]; N % 4 == 0.
 *
 * dfx_conv1x1_pair_f32: Y[n] = act(W x [X1[n] ; X2[n]] + bias) - two NCHW inputs of the same map size concatenated
 * along the channels INSIDE the product: the last 1x1 convolution of a bottleneck and the stride-1 projection
 * shortcut of the same block (torchvision Bottleneck: out = relu(bn3(conv3(t)) + downsample(x)),
 * /root/reference/models/backbone_scratch.py:102-141 via resnet50's layer1[0] and the dilated layer4[0]) as ONE GEMM
 * with W = [W3 | Wd] (frozen-BN scales folded in, bias = shift3 + shiftd): the shortcut map is neither written nor
 * read back as a residual.  X1 [batch,K1,HW], X2 [batch,K2,HW] (image strides in floats), W [Co,K1+K2] row-major,
 * Y [batch,Co,HW]; K1, K2 multiples of 16, HW of 4.
 *
 * dfx_conv1x1_chain_f32: a bottleneck's last 1x1 convolution AND the first 1x1 convolution of the block that follows it
 * (torchvision Bottleneck, /root/reference/models/backbone_scratch.py:102-141: the stride sits on conv2, so every conv1 is a
 * stride-1 product over the map its predecessor wrote) in one launch:
 *   Y[n] = relu(W3 x [X1[n] ; X2[n]] + b3 + R[n])     [Co, HW]
 *   Z[n] = act_z(W1 x Y[n] + b1)                      [C1, HW]   act_z 0: none, 1: ReLU
 * Z is computed from the Y tile while it is still in registers: the Co-channel map is written once and not read back.
 * X2 (with K2 > 0: the two-segment form of dfx_conv1x1_pair_f32), R, b3 and b1 are optional (NULL; K2 = 0 without X2).
 * W3 [Co, K1+K2], W1 [C1, Co] row-major; X1 [batch,K1,HW], X2 [batch,K2,HW], R and Y [batch,Co,HW], Z [batch,C1,HW] with
 * image strides in floats.  Covered: Co, C1 and K1+K2 multiples of 32 (K1, K2 of 16), K1+K2 <= 128, C1 <= 256 (the
 * activation panel and the Z accumulators of a wave live in registers), HW a multiple of 4; any other shape returns
 * DFX_EINVAL without a launch and the caller runs the two products as separate calls.  Y and Z are bit-equal to
 * dfx_gemm_f32 / dfx_conv1x1_pair_f32 followed by dfx_gemm_f32 on the same operands (same k order, same epilogue order).
 *
 * dfx_gemm_wgrad_f32: the weight and bias gradients of y = x W^T + b (csrc/gemm_wgrad.hip), what autograd computes for the
 * nn.Linear layers listed above when they train:
 *   dW[n][k] = sum_m dY[m][n] X[m][k]     [N, K], row pitch ldw
 *   db[n]    = sum_m dY[m][n]             [N]; db may be NULL and is then not computed
 * dY [M, N] (ldy) and X [M, K] (ldx) row-major: both operands are k-major for this product, whose summed dimension is the row
 * count M.  Exact fp32 MFMA.  The outputs are overwritten, never accumulated into.  M is cut into ``splits`` ranges of whole
 * 16-row steps (``splits`` is clamped so that no range is empty); with more than one range the partial results go to
 * ``workspace`` (splits * (N * K + N) floats, caller-owned, 16-byte aligned) and one reduction launch adds them in ascending
 * range order: no atomics, two calls give the same bits.  One range stores directly and ``workspace`` may be NULL.  db comes
 * from the dY values the product stages anyway: no second pass over dY.
 * N, K, ldy, ldx and ldw multiples of 4 (ld >= the row), dY, X, dW and workspace 16-byte aligned, else DFX_EINVAL.  Only one
 * range has to stay below 2 GiB (rows per range * max(ldy, ldx) * 4 bytes, else DFX_ERANGE); the operands may be larger.
 * N * K == 0 returns DFX_OK without a launch; M == 0 writes zeros to dW and db.
 *
 * dfx_conv1x1_wgrad_f32: the weight gradient of a 1x1 convolution Z[n] = W x X[n] (the input projections, Conv2d(2048, 256, 1)
 * and Conv2d(128, 256, 1), /root/reference/models/deformable_detr_single.py:101-125, when they train):
 *   dW[co][ci] = sum_n sum_p dZ[n][co][p] X[n][ci][p]     [Co, Ci] packed
 * dZ [batch,Co,HW], X [batch,Ci,HW] with image strides in floats.  It is the b_is_kn = 0 product of dfx_gemm_splitk_f32
 * with the batch turned on: ONE product launch over images x pixel ranges of whole 16-deep steps (``splits`` ranges per
 * image, clamped so that none is empty) writes partial [Co,Ci] slabs to ``workspace`` (batch * splits * Co * Ci floats,
 * caller-owned, 16-byte aligned), one reduction launch adds them in ascending (image, range) order: no atomics, two calls
 * give the same bits, dW is overwritten.  A single image in a single range stores directly and ``workspace`` may be NULL.
 * Co, Ci, HW and the strides multiples of 4, dZ, X, dW and workspace 16-byte aligned, else DFX_EINVAL; one image's operand
 * (and dW) must stay below 2 GiB, batch * splits at most 65535, else DFX_ERANGE.  Co * Ci == 0 returns DFX_OK without a
 * launch; batch * HW == 0 writes zeros to dW.
 */
#ifndef DFX_GEMM_H
#define DFX_GEMM_H

#ifdef __cplusplus
extern "C" {
#endif

int dfx_gemm_f32(const float *A, const float *A2, long lda, long strideA,
                 const float *B, long ldb, long strideB, int b_is_kn,
                 const float *bias, int bias_per_row,
                 const float *R, long ldr, long strideR,
                 const unsigned char *row_mask, long strideMask,
                 float *C, long ldc, long strideC,
                 int M, int N, int K, int batch, int relu,
                 int c_block, long c_block_stride, long a_block_stride, void *stream);

int dfx_gemm_splitk_f32(const float *A, long lda, const float *B, long ldb, int b_is_kn,
                        const float *bias, int bias_per_row, const float *R, long ldr,
                        float *C, long ldc, int M, int N, int K, int act, int splits,
                        float *workspace, void *stream);

int dfx_conv1x1_pair_f32(const float *W, const float *X1, long strideX1, int K1,
                         const float *X2, long strideX2, int K2, const float *bias,
                         float *Y, long strideY, int Co, int HW, int batch, int act, void *stream);

int dfx_conv1x1_chain_f32(const float *W3, const float *X1, long strideX1, int K1,
                          const float *X2, long strideX2, int K2, const float *b3,
                          const float *R, long strideR, float *Y, long strideY,
                          const float *W1, const float *b1, float *Z, long strideZ,
                          int Co, int C1, int HW, int batch, int act_z, void *stream);

int dfx_gemm_wgrad_f32(const float *dY, long ldy, const float *X, long ldx,
                       float *dW, long ldw, float *db,
                       int M, int N, int K, int splits, float *workspace, void *stream);

int dfx_conv1x1_wgrad_f32(const float *dZ, long strideZ, const float *X, long strideX, float *dW,
                          int Co, int Ci, int HW, int batch, int splits, float *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_GEMM_H */
