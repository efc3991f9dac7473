/*
 * dfx_msda.h -- C ABI of the MI355X (gfx950) multi-scale deformable attention path.
 *
 * This is the drop-in boundary: the entry points are exactly what a binding for
 * the reference's only native component would call.  The reference exposes that
 * component as the pybind11 module `MultiScaleDeformableAttention` with
 *   ms_deform_attn_forward   /root/reference/models/ops/src/ms_deform_attn.h:20-38
 *   ms_deform_attn_backward  /root/reference/models/ops/src/ms_deform_attn.h:41-61
 * (bound in models/ops/src/vision.cpp:13-16, implemented for CUDA in
 *  models/ops/src/cuda/ms_deform_attn_cuda.cu:20-153).  The Python shim that
 * turns these C calls back into that module lives in
 *   depth-fusion-in-transformer-based-video-object-detection_amd/MultiScaleDeformableAttention.py
 * and INTEGRATION.md shows the few lines a maintainer of the reference adds.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; no torch / ATen types cross this boundary;
 *   - every pointer is DEVICE memory (HBM) of the current HIP device, including
 *     `shapes` and `lsi` (the reference keeps them on the device as int64);
 *   - buffers are packed, row-major, and addressed FLAT with strides derived
 *     from the integer arguments (ms_deform_attn_cuda.cu:40-48,58-60): a
 *     sampling-location buffer that is larger than N*Lq*M*L*P*2 is legal and
 *     only its prefix is read (the TransVOD temporal decoder relies on this);
 *   - the call only ENQUEUES work on `stream` (a hipStream_t; NULL = the
 *     default stream) and returns; no allocation, no synchronisation, no global
 *     state, re-entrant;
 *   - the caller owns every buffer; outputs are fully overwritten by forward;
 *     backward ACCUMULATES (atomic adds) into grad_value, grad_loc and grad_aw,
 *     so the caller zero-fills all three first (the reference allocates them
 *     with zeros_like, ms_deform_attn_cuda.cu:116-118);
 *   - return value: 0 on success, a negative DFX_E* code otherwise; no C++
 *     exception ever crosses the boundary; dfx_last_error() gives the text.
 */
#ifndef DFX_MSDA_H
#define DFX_MSDA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_OK 0
#define DFX_EINVAL (-1)  /* bad dimension / null pointer                         */
#define DFX_ELAUNCH (-2) /* hipGetLastError() reported a launch failure          */
#define DFX_ERANGE (-3)  /* sizes overflow the 32-bit index space of the kernels */

/* ABI version: bumped whenever a signature changes or an exported symbol goes away. */
int dfx_abi_version(void);

/* Text of the last error raised on the calling thread ("" if none). */
const char *dfx_last_error(void);

/*
 * Measurement aid (bench.py); not part of the reference's surface and the one place with process-wide
 * state.  While enabled, every fused MSDA kernel, every GEMM and every convolution launch is dispatched with
 * hipExtLaunchKernelGGL, which stamps an event pair with the kernel's own begin / end timestamps (the kernel
 * duration proper, on the launch stream, without the dispatch gap of hipEventRecord pairs).
 * dfx_profile_drain waits for the recorded kernels, writes up to `cap` records, frees the events and returns
 * the number written.  Record = (duration in ms, work, tag_a, tag_b):
 *   MSDA kernels      work = algorithmic bytes of the launch, tag_a = Lq (> 0), tag_b = S
 *   gemm_f32_kernel   work = 2*M*N*K*batch flops, tag_a = -1 ([K,N] operand: 1x1 convolution) / -2 (Linear), tag_b = tile
 *   conv_wino_kernel  work = MFMA flops executed (2*16*Co*Ci per 2x2 tile), tag_a = -3, tag_b = dilation
 *   conv_igemm_kernel work = 2*Co*Kpad*Ho*Wo*N flops, tag_a = -4, tag_b = tile rows
 */
int dfx_profile_enable(int on);
int dfx_profile_drain(float *ms, long *bytes, int *lq, int *s, int cap);

/*
 * The launchers' DFX_* tuning / diagnostic environment switches are read once per process;
 * this re-reads them (A/B tools and tests that change the environment of a running process).
 */
int dfx_tuning_reload(void);

/*
 * Forward: out[b,q,m,c] = sum_{l,p} aw[b,q,m,l,p] * bilinear(value_l[b,:,m,c], x*W_l-0.5, y*H_l-0.5)
 * Replaces ms_deform_attn_cuda_forward (ms_deform_attn_cuda.cu:20-80) and the
 * kernel ms_deformable_im2col_gpu_kernel (ms_deform_im2col_cuda.cuh:237-299).
 *   value  [N,S,M,D]        shapes int64 [L,2] = (H_l, W_l)      lsi int64 [L]
 *   loc    >= N*Lq*M*L*P*2  aw >= N*Lq*M*L*P                     out [N,Lq,M*D]
 */
int dfx_msda_forward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                         const float *loc, const float *aw,
                         int N, int S, int M, int D, int L, int Lq, int P,
                         float *out, void *stream);
int dfx_msda_forward_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                         const double *loc, const double *aw,
                         int N, int S, int M, int D, int L, int Lq, int P,
                         double *out, void *stream);

/*
 * Backward.  Replaces ms_deform_attn_cuda_backward (ms_deform_attn_cuda.cu:83-153)
 * and the six col2im kernel variants (ms_deform_im2col_cuda.cuh:301-920).
 *   grad_out [N,Lq,M*D]; grad_value like value; grad_loc like loc; grad_aw like aw.
 */
int dfx_msda_backward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *aw, const float *grad_out,
                          int N, int S, int M, int D, int L, int Lq, int P,
                          float *grad_value, float *grad_loc, float *grad_aw, void *stream);
int dfx_msda_backward_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                          const double *loc, const double *aw, const double *grad_out,
                          int N, int S, int M, int D, int L, int Lq, int P,
                          double *grad_value, double *grad_loc, double *grad_aw, void *stream);

/*
 * 2-byte value maps (mixed precision: what MSDeformAttn hands the operator under torch.autocast).
 * value, grad_out and out are bf16 (the _bf16 pair) or IEEE fp16 (the _f16 pair), passed as raw
 * 16-bit words; loc and aw are fp32 in every case.  The arithmetic is the fp32 operator's (corner
 * weights, products and the sum over L*P samples in fp32), and each output element is rounded once
 * to the value's type.  Backward accumulates into three zero-filled fp32 buffers: grad_value_f32 is
 * laid out like value ([N,S,M,D] floats) and the caller rounds it to the value's type.
 * Replaces the same reference lines as the fp32 pairs above (which dispatch fp32 / fp64 only,
 * AT_DISPATCH_FLOATING_TYPES, ms_deform_attn_cuda.cu:64,136).
 */
int dfx_msda_forward_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *aw, int N, int S, int M, int D, int L, int Lq, int P,
                          uint16_t *out, void *stream);
int dfx_msda_backward_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *aw, const uint16_t *grad_out,
                           int N, int S, int M, int D, int L, int Lq, int P,
                           float *grad_value_f32, float *grad_loc, float *grad_aw, void *stream);
int dfx_msda_forward_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                         const float *loc, const float *aw, int N, int S, int M, int D, int L, int Lq, int P,
                         uint16_t *out, void *stream);
int dfx_msda_backward_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *aw, const uint16_t *grad_out,
                          int N, int S, int M, int D, int L, int Lq, int P,
                          float *grad_value_f32, float *grad_loc, float *grad_aw, void *stream);

/*
 * Fused front end + sampling (inference): what MSDeformAttn.forward does between
 * its Linear layers (/root/reference/models/ops/modules/ms_deform_attn.py:98-114):
 *   aw  = softmax over (L*P) of logits[b,q,m,:]
 *   loc = ref[b,q,l,:2] + off[b,q,m,l,p,:] / (W_l,H_l)                (ref_dim == 2)
 *   loc = ref[b,q,l,:2] + off[b,q,m,l,p,:] / P * ref[b,q,l,2:] * 0.5  (ref_dim == 4)
 * followed by the forward above, without materialising loc / aw in HBM.
 *   off    [N,Lq,M,L,P,2] raw sampling_offsets Linear output, row stride
 *          `off_stride` floats between consecutive (b,q) rows (>= M*L*P*2)
 *   logits [N,Lq,M,L*P]   raw attention_weights Linear output, row stride
 *          `logit_stride` floats (>= M*L*P); both strides let one GEMM write a
 *          concatenated [offsets | logits] row
 *   ref    [N,Lq,Lr,ref_dim]; Lr == L normally.  Lr > L reproduces the flat
 *          read of the TransVOD temporal decoder: the
 *          virtual location tensor [Lq,M,Lr,P,2] of EACH batch element is read
 *          flat with L levels (the reference only does this with N == 1; for
 *          N > 1 every batch element follows the N == 1 rule on its own).
 */
int dfx_msda_fused_forward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                               const float *ref, int ref_dim, int Lr,
                               const float *off, long off_stride,
                               const float *logits, long logit_stride,
                               int N, int S, int M, int D, int L, int Lq, int P,
                               float *out, void *stream);

/*
 * Backward of dfx_msda_fused_forward_f32 (training; csrc/msda_fused_backward.hip) from the forward's own raw
 * inputs: the kernel recomputes the softmax weights and the locations, the caller saves nothing else.
 * Replaces ms_deform_attn_cuda_backward (ms_deform_attn_cuda.cu:83-153) together with what autograd runs
 * behind it for the reference's models/ops/modules/ms_deform_attn.py:98-110 (softmax, divide, broadcast add).
 * Geometry of the fused forward (fp32, M = 8, D = 32, P = 4, 1 <= L <= 4, ref_dim 2 or 4) with Lr == L only;
 * the same argument checks (strides multiples of 4 and not smaller than the row, 16-byte alignment, sizes).
 *   grad_out    [N,Lq,M*D]
 *   grad_value  [N,S,M,D] ACCUMULATED into with float atomics: the caller zero-fills it.  May be NULL (the
 *               memory needs no gradient): the kernel then contains no atomics at all.
 *   grad_off    like off, row stride grad_off_stride      \  WRITTEN in full with plain stores (every element
 *   grad_logits like logits, row stride grad_logit_stride  > has one owning wave): the caller need not
 *   grad_ref    [N,Lq,L,ref_dim], may be NULL             /  initialise them; two calls give the same bits.
 * N*Lq == 0 returns DFX_OK without a launch; S == 0 writes zeros to the three small
 * gradients.  An addition to the ABI: dfx_abi_version() stays.
 */
int dfx_msda_fused_backward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                                const float *ref, int ref_dim,
                                const float *off, long off_stride,
                                const float *logits, long logit_stride,
                                const float *grad_out,
                                int N, int S, int M, int D, int L, int Lq, int P,
                                float *grad_value,
                                float *grad_off, long grad_off_stride,
                                float *grad_logits, long grad_logit_stride,
                                float *grad_ref,
                                void *stream);

/*
 * The same fused operator for single-level attention with the whole level resident in LDS
 * (csrc/msda_level.hip): L = 1, one reference level, P = 4, M = 8, D = 32, any Lq.  A workgroup
 * stages 8 channels of one head of every token of the H x W map (zero-bordered) into LDS and the
 * bilinear gathers never leave the CU.  H and W are HOST integers (the LDS image is sized from
 * them); the level must fit: dfx_msda_fused_level_fits(H, W) != 0, i.e. (H+3)*(W+2)*32 B within
 * the CU's 160 KB (50 x 84 at 800 x 1333 does).  Results equal dfx_msda_fused_forward_f32 up to
 * rounding (softmax and the location quotient are computed with correctly rounded divisions, the
 * exponential to 1 ulp).  Replaces the same reference lines as dfx_msda_fused_forward_f32
 * (models/ops/modules/ms_deform_attn.py:98-114).
 *
 * Operands are addressed through dfx_msda_level_layout (strides in floats, multiples of 4):
 *   value   channel c of head m of token s of frame n at
 *           value[n*value_frame + s*value_token + m*value_head + (c/8)*value_oct + ((c/4)%2)*value_chunk + c%4]
 *           reference layout [N,S,8,32]: (S*256, 256, 32, 8, 4); the layout the kernel is built for is
 *           dfx_gemm_f32's c_block = 4 output [64][N*S][4]: (S*4, 4, 32*N*S, 8*N*S, 4*N*S), where every
 *           16-byte chunk plane a workgroup stages is contiguous
 *   off     the 4 (x, y) offsets of head m of query row r = n*Lq + q at off[r*off_row + m*off_head + 0..7]
 *   logits  its 4 attention logits at logits[r*logit_row + m*logit_head + 0..3]
 *           reference Linear outputs: off (64-float rows, head stride 8), logits (32-float rows, head
 *           stride 4); built-for layout: one c_block = 12 GEMM output [8][N*Lq][12] holding
 *           (offsets, logits) of a head side by side: off_row = logit_row = 12,
 *           off_head = logit_head = N*Lq*12, logits = off + 8
 *   out     channel c of head m of query row r at
 *           out[r*out_row + m*out_head + (c/8)*out_oct + ((c/4)%2)*out_chunk + c%4]
 *           reference layout [N,Lq,256]: (256, 32, 8, 4); built-for layout [64][N*Lq][4]
 *           (dfx_gemm_f32's K-block-major A operand of output_proj): (4, 32*N*Lq, 8*N*Lq, 4*N*Lq)
 *   ref [N,Lq,1,ref_dim]
 */
typedef struct dfx_msda_level_layout {
    long value_frame, value_token, value_head, value_oct, value_chunk;
    long off_row, off_head, logit_row, logit_head;
    long out_row, out_head, out_oct, out_chunk;
} dfx_msda_level_layout;

int dfx_msda_fused_level_fits(int H, int W);
int dfx_msda_fused_level_forward_f32(const float *value, const float *ref, int ref_dim,
                                     const float *off, const float *logits,
                                     const dfx_msda_level_layout *layout,
                                     int N, int H, int W, int Lq, float *out, void *stream);

/*
 * grad_value of the single-level fused operator, summed in LDS (training; csrc/msda_level_backward.hip): the value
 * gradient of dfx_msda_fused_backward_f32 for L = 1, M = 8, D = 32, P = 4, fp32 and a level that fits
 * (dfx_msda_fused_level_fits(H, W) != 0), without a global atomic.  One workgroup owns a (frame, head, channel octet)
 * slice of grad_value, sums the contributions of ALL queries of the frame into an LDS image of the level and stores
 * the finished slice once.  Together with dfx_msda_fused_backward_f32 called with grad_value == NULL (the three small
 * gradients, no atomics) it is the whole backward of a single-level layer.  Replaces the grad_value part of
 * ms_deform_attn_cuda_backward (ms_deform_attn_cuda.cu:83-153; the atomicAdd of ms_deform_im2col_cuda.cuh:301-920).
 * Reference layouts only, pointers plus row pitches in floats as dfx_msda_fused_backward_f32 takes them:
 *   ref        [N,Lq,1,ref_dim], ref_dim 2 or 4, 16-byte aligned (8 for ref_dim 2)
 *   off        [N,Lq,64] raw sampling_offsets rows, `off_pitch` floats apart (>= 64, a multiple of 4)   \  16-byte aligned;
 *   logits     [N,Lq,32] raw attention_weights rows, `logit_pitch` floats apart (>= 32, a multiple of 4) / may be column
 *              slices of one wider buffer
 *   grad_out   [N,Lq,256] contiguous
 *   grad_value [N,H*W,8,32] contiguous, WRITTEN in full with plain 16-byte stores (every element has one writer, zeros
 *              included): the caller need not initialise it.
 * All argument checks run before any launch.  N == 0 returns DFX_OK without a launch; Lq == 0 with N > 0 writes zeros
 * to grad_value.  N*Lq < 2^28.  The softmax and the sampling locations are the level forward's arithmetic.
 * NOT bit-reproducible in the default mode: the order of the LDS float adds is not fixed, so two calls may differ in the
 * last bits - as the global-atomic grad_value of dfx_msda_fused_backward_f32; the _fixed_ entry points below are.
 * An addition to the ABI: dfx_abi_version() stays.
 */
int dfx_msda_level_grad_value_f32(const float *ref, int ref_dim,
                                  const float *off, long off_pitch,
                                  const float *logits, long logit_pitch,
                                  const float *grad_out,
                                  int N, int H, int W, int Lq,
                                  float *grad_value, void *stream);

/*
 * Deterministic grad_value (csrc/fixed_sum.h): the two entry points above with every contribution - the float route's
 * own fp32 product - scaled by a power of two taken from max |grad_out| of the launch, rounded to a 64-bit integer and
 * summed with integer atomics.  Integer addition is associative: grad_value has the same bits from call to call and
 * under any permutation of the queries.  Scaling grad_out by a power of two scales grad_value by it exactly.
 *   scratch     16 bytes, 16-byte aligned, caller-owned; the entry point clears it and leaves the bit pattern of
 *               max |grad_out| in its first word.  The host never reads it.
 *   workspace   (the fused form) N*S*M*D 64-bit integers laid out like grad_value, 16-byte aligned, ZERO-FILLED by the
 *               caller; holds the sums after the call.
 *   grad_value  WRITTEN in full by both forms (the caller need not initialise it); the fused form requires it - for the
 *               three small gradients alone call dfx_msda_fused_backward_f32 with grad_value == NULL, which has no atomics.
 * grad_off, grad_logits and grad_ref of the fused form are the bits of dfx_msda_fused_backward_f32.
 * max |grad_out| == 0, Lq == 0: exact zeros.  ANY inf or NaN in grad_out makes EVERY element of grad_value NaN.
 * dfx_msda_fixed_fraction_bits(Lq): the fraction bits F = min(50, 61 - ceil(log2(16 * Lq))) both forms use (16 * Lq
 * bounds the (query, point, corner) triples that can meet in one element).
 * Otherwise the argument rules, checks (all before any launch) and geometry of the float entry points.
 * Additions to the ABI: dfx_abi_version() stays.
 */
int dfx_msda_fixed_fraction_bits(int Lq);
int dfx_msda_level_grad_value_fixed_f32(const float *ref, int ref_dim,
                                        const float *off, long off_pitch,
                                        const float *logits, long logit_pitch,
                                        const float *grad_out,
                                        int N, int H, int W, int Lq,
                                        float *grad_value, void *scratch, void *stream);
int dfx_msda_fused_backward_fixed_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                                      const float *ref, int ref_dim,
                                      const float *off, long off_stride,
                                      const float *logits, long logit_stride,
                                      const float *grad_out,
                                      int N, int S, int M, int D, int L, int Lq, int P,
                                      float *grad_value, long long *workspace, void *scratch,
                                      float *grad_off, long grad_off_stride,
                                      float *grad_logits, long grad_logit_stride,
                                      float *grad_ref,
                                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_MSDA_H */
