/*
 * dfx_roi.h -- C ABI of the RoIAlign used by the TransVOD++ query/RoI fusion stage.
 *
 * Replaces the third-party op the reference calls on this path:
 *   mmcv.ops.RoIAlign(output_size=7, spatial_scale=1/32, sampling_ratio=2)   (mmcv-full 1.7.0,
 *   pool_mode='avg', aligned=True), constructed at
 *   /root/reference/models/deformable_transformer_multi_plusplus.py:129-132 and called at :499,:514.
 * mmcv is not vendored in the reference and holds no test there: parity is pinned to this
 * repository's own restatement of the published algorithm (oracle/msda_oracle.c).
 *
 * Same conventions as dfx_msda.h: device pointers, caller-owned buffers, enqueue-only on
 * `stream`, 0 / negative return code.
 *   rois [K,5] = (batch index, x1, y1, x2, y2) in input-image pixels (scaled by spatial_scale).
 */
#ifndef DFX_ROI_H
#define DFX_ROI_H

#ifdef __cplusplus
extern "C" {
#endif

/* input [N,C,H,W] -> out [K,C,ph,pw]  (the layout mmcv works in) */
int dfx_roi_align_nchw_f32(const float *input, const float *rois, int N, int C, int H, int W, int K,
                           int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                           float *out, void *stream);

/* input [N,H,W,C] (token-major encoder memory, no transpose needed) -> out [K,ph*pw,C];
 * C must be a multiple of 4 and both buffers 16-byte aligned. */
int dfx_roi_align_nhwc_f32(const float *input, const float *rois, int N, int C, int H, int W, int K,
                           int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                           float *out, void *stream);

/* Backward of the two entry points above: the transpose of the forward map, for the feature map only (the RoIs get
 * no gradient, as in the published mmcv op).  grad_out has the forward's output layout, grad_input the forward's
 * input layout.  Unlike dfx_msda_backward_* the entry point zero-fills grad_input [N*C*H*W floats] itself on
 * `stream` before it accumulates into it with fp32 atomic adds (also when K == 0, where it then returns), so
 * in the default mode sums may differ in the last bits from run to run.  Samples the forward skips, and RoIs whose batch index is
 * outside [0, N), contribute nothing.  Same argument rules as the forward; nhwc: C a multiple of 4, grad_out and
 * grad_input 16-byte aligned.  Additions to the ABI: no existing signature changes, dfx_abi_version() stays. */
int dfx_roi_align_backward_nchw_f32(const float *grad_out, const float *rois, int N, int C, int H, int W, int K,
                                    int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                    float *grad_input, void *stream);

int dfx_roi_align_backward_nhwc_f32(const float *grad_out, const float *rois, int N, int C, int H, int W, int K,
                                    int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                    float *grad_input, void *stream);

/* Deterministic NHWC backward (csrc/fixed_sum.h): dfx_roi_align_backward_nhwc_f32 with every contribution - the float
 * route's own fp32 product - scaled by a power of two taken from max |grad_out|, rounded to a 64-bit integer and summed
 * with integer atomics, so grad_input has the same bits from call to call and under any permutation of the RoIs.
 *   workspace  N*H*W*C 64-bit integers laid out like grad_input, 16-byte aligned, ZERO-FILLED by the caller
 *   scratch    16 bytes, 16-byte aligned, caller-owned; cleared by the call, then holds the bit pattern of max |grad_out|
 * grad_input is written in full.  max |grad_out| == 0 or K == 0: exact zeros; ANY inf or NaN in grad_out makes EVERY
 * element NaN.  dfx_roi_align_fixed_fraction_bits: F = min(50, 61 - ceil(log2(4 * sr^2 * ph * pw * K))), the bound being
 * the (RoI, bin, sample, corner) terms that can meet in one pixel; a launch whose bound reaches 2^32 is refused.
 * The adaptive grid (sampling_ratio <= 0) has no host bound and is refused like everywhere on this path.
 * Additions to the ABI: dfx_abi_version() stays. */
int dfx_roi_align_fixed_fraction_bits(int K, int ph, int pw, int sampling_ratio);
int dfx_roi_align_backward_nhwc_fixed_f32(const float *grad_out, const float *rois, int N, int C, int H, int W, int K,
                                          int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                          float *grad_input, long long *workspace, void *scratch, void *stream);

/* DynamicConv of the query/RoI fusion head (Sparse R-CNN instance interaction) between the parameter
 * Linear and the output Linear, one launch (/root/reference/models/sparse_roi_head/head.py:98-113):
 *   k1 = params[r, 0 : C*dd] as [C,dd];  k2 = params[r, C*dd : 2*C*dd] as [dd,C]
 *   y  = relu(LayerNorm_dd(feats[r] @ k1));   out[r] = relu(LayerNorm_C(y @ k2))
 * for every RoI r: feats / out [K,R,C] (R = ph*pw <= 64 rows), params [K, >= 2*C*dd] with row stride
 * p_stride (the dynamic_layer output as it stands), C = 256, dd = 64, eps 1e-5 inside the sqrt.
 * The library runs this as two batched GEMMs of 49-row matrices plus four normalisation / ReLU passes
 * over [K,R,C]; here each RoI's matrices stay in one CU's LDS between the two fp32-MFMA products. */
int dfx_dynamic_conv_f32(const float *feats, const float *params, long p_stride,
                         const float *g1, const float *b1, const float *g2, const float *b2,
                         float *out, int K, int R, int C, int dd, float eps, void *stream);

/* Backward of dfx_dynamic_conv_f32 from its inputs alone: the kernel recomputes the forward's intermediates per RoI
 * (csrc/dynconv_backward.hip), nothing is saved between the two calls.  grad_out [K,R,C] is the gradient of `out`.
 *   grad_feats  [K,R,C]           gradient of feats; null: not computed (its product and stores are skipped)
 *   grad_params [K, >= 2*C*dd]    row stride gp_stride; columns 0 .. 2*C*dd of every row are written (dK1 then dK2),
 *                                 columns beyond are not touched; null: not computed
 *   grad_ln     [2*dd + 2*C]      dg1[dd] db1[dd] dg2[C] db2[C], summed over all K*R rows, always written
 *   workspace   DFX_DYNCONV_BWD_WS_FLOATS floats, caller-owned, contents irrelevant before and after the call
 * No atomics: every workgroup sums its own LayerNorm parameter gradients into one workspace row and a second kernel
 * adds the rows in order, so for given K the results are bit-identical from run to run.  Same argument rules and
 * geometry as the forward (C = 256, dd = 64, R <= 64, 16-byte aligned buffers, strides multiples of 4);  K == 0
 * zero-fills grad_ln and returns.  An addition to the ABI: dfx_abi_version() stays. */
#define DFX_DYNCONV_BWD_WS_FLOATS (256 * 640)
int dfx_dynamic_conv_backward_f32(const float *grad_out, const float *feats, const float *params, long p_stride,
                                  const float *g1, const float *b1, const float *g2, const float *b2,
                                  float *grad_feats, float *grad_params, long gp_stride, float *grad_ln,
                                  float *workspace, int K, int R, int C, int dd, float eps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_ROI_H */
