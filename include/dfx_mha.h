/*
 * dfx_mha.h -- C ABI of the fused scaled-dot-product attention of the 300-query layers (gfx950).
 *
 * It stands where the reference calls torch.nn.MultiheadAttention on this path (always without masks,
 * dropout off in eval): the object-query self-attention of every decoder layer
 *   /root/reference/models/deformable_transformer_single.py:650-655 (DeformableTransformerDecoderLayer)
 * the TQE self- and cross-attention and the TDTD self-attention of the temporal stage
 *   /root/reference/models/deformable_transformer_multi_plusplus.py:815-838, 879-886
 * and the RCNNHead self-attention of the query/RoI fusion
 *   /root/reference/models/sparse_roi_head/head.py:70-76.
 * The in/out projections stay GEMMs (dfx_gemm_f32); this call is the part in between, which the
 * library path runs as  q*scale, two transposing copies, bmm, softmax, bmm, copy  (7-9 launches):
 *
 *   out[b,i,h*32+d] = sum_j softmax_j( scale * <q[b,i,h,:], k[b,j,h,:]> ) * v[b,j,h,d]
 *
 * fp32 (exact-fp32 MFMA, online softmax), head dimension 32, `heads` heads side by side in the last
 * dimension (E = 32*heads).  q [B,Lq,E], k / v [B,Lk,E], out [B,Lq,E]: the last dimension is
 * contiguous, batch and sequence strides are given in floats (multiples of 4), so q / k / v may be
 * column slices of one joint projection output.  Same conventions as dfx_msda.h (device pointers,
 * enqueue-only, 0 / <0).
 *
 * Training (the same layers in grad mode, where the module also drops attention probabilities):
 *
 *   dfx_mha_train_forward_f32  is dfx_mha_f32 with two more operands (the same kernel body, compile-time flags):
 *     lse  [B,heads,Lq] fp32 contiguous, output:  lse[b,h,i] = ln sum_j exp(scale * <q_i, k_j>)  (natural log)
 *     drop [B,heads,Lq,Lk] fp32 contiguous, 16-byte aligned, input or NULL: multiplies the normalised probabilities
 *          (0 or 1/(1-p));  out = sum_j softmax_ij * drop_ij * v_j, the denominator is the undropped sum.
 *     With drop == NULL `out` has the bits of dfx_mha_f32.  Any Lk.
 *
 *   dfx_mha_backward_f32  recomputes P = exp(scale * S - lse) tile by tile and, with delta_i = <dO_i, O_i>,
 *     dP = (dO V^T) o drop,  dS = scale * P o (dP - delta),  dV = (P o drop)^T dO,  dQ = dS K,  dK = dS^T Q.
 *     grad_out, q, k, v, out and the gradients are (pointer, batch stride, row stride) like the forward's operands;
 *     lse and drop as above.  grad_q may be NULL, grad_k and grad_v may be NULL together: that work is not done.
 *     One launch, no atomics (every gradient element is owned by one wave): outputs need no zero fill, and two calls
 *     give the same bits.  Nothing of size Lq x Lk is read except drop, nothing of that size is written.
 */
#ifndef DFX_MHA_H
#define DFX_MHA_H

#ifdef __cplusplus
extern "C" {
#endif

int dfx_mha_f32(const float *q, long q_batch, long q_row,
                const float *k, long k_batch, long k_row,
                const float *v, long v_batch, long v_row,
                float *out, long o_batch, long o_row,
                int B, int heads, int Lq, int Lk, float scale, void *stream);

int dfx_mha_train_forward_f32(const float *q, long q_batch, long q_row,
                              const float *k, long k_batch, long k_row,
                              const float *v, long v_batch, long v_row,
                              float *out, long o_batch, long o_row,
                              float *lse, const float *drop,
                              int B, int heads, int Lq, int Lk, float scale, void *stream);

int dfx_mha_backward_f32(const float *grad_out, long go_batch, long go_row,
                         const float *q, long q_batch, long q_row,
                         const float *k, long k_batch, long k_row,
                         const float *v, long v_batch, long v_row,
                         const float *out, long o_batch, long o_row,
                         const float *lse, const float *drop,
                         float *grad_q, long gq_batch, long gq_row,
                         float *grad_k, long gk_batch, long gk_row,
                         float *grad_v, long gv_batch, long gv_row,
                         int B, int heads, int Lq, int Lk, float scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_MHA_H */
