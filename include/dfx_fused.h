/*
 * dfx_fused.h -- C ABI of the fused elementwise epilogues around the convolutions / GEMMs that
 * feed the deformable-attention path.
 *
 * The reference runs these as separate PyTorch kernels:
 *   FrozenBatchNorm2d.forward   x * scale + bias        /root/reference/models/backbone_scratch.py:58-68
 *   Bottleneck tail             out += identity; relu   (torchvision resnet50, used at backbone_scratch.py:156-159)
 * With the frozen statistics folded into the convolution weights (scale) the remaining work per
 * convolution is one pass:  y = act(x + bias[c] (+ residual)).
 *
 * Same conventions as dfx_msda.h (device pointers, caller-owned buffers, enqueue-only, 0 / <0).
 */
#ifndef DFX_FUSED_H
#define DFX_FUSED_H

#ifdef __cplusplus
extern "C" {
#endif

/* x, residual (may be NULL), out: [N,C,HW] packed (NCHW); bias [C]; out may alias x.
 * out = relu?( x + bias[c] + residual ) */
int dfx_bias_act_nchw_f32(const float *x, const float *bias, const float *residual, float *out,
                          int N, int C, long HW, int relu, void *stream);

/* ResNet stem epilogue in one pass: out = maxpool3x3/s2/p1( relu(x + bias[c]) ), NCHW.
 * Replaces FrozenBatchNorm2d (shift; the scale is folded into conv1) + ReLU + nn.MaxPool2d of the stem
 * (/root/reference/models/backbone_scratch.py:112-115).  x [N,C,H,W] -> out [N,C,(H+1)/2,(W+1)/2]. */
int dfx_bias_relu_maxpool_f32(const float *x, const float *bias, float *out, int N, int C, int H, int W,
                              void *stream);

/* Residual add + LayerNorm over the last dimension in one pass (the reference runs ``norm(x + y)`` as an
 * add kernel followed by nn.LayerNorm: deformable_transformer_single.py:556-562 and every other block):
 *   out[r,:] = LayerNorm(x[r,:] (+ res[r,:])) * gamma + beta,  biased variance, eps inside the sqrt.
 * x, res (may be NULL), out: [rows, C] packed fp32; C a multiple of 4, C <= 1024; out may alias x. */
int dfx_add_layernorm_f32(const float *x, const float *res, const float *gamma, const float *beta, float *out,
                          long rows, int C, float eps, void *stream);

/* The same tail under a training step, with the sub-layer's dropout (csrc/layernorm_train.hip):
 *   s[r,:] = res[r,:] + x[r,:] * mask[r,:],   out[r,:] = LayerNorm(s[r,:]) * gamma + beta
 * in dfx_add_layernorm_f32's arithmetic and order: without a mask ``out`` has that entry's bits, with one the bits of that
 * entry run on x * mask (the product is rounded before the add).  Also written, for the backward: s [rows,C], mean and
 * rstd [rows] each (rstd the correctly rounded 1 / sqrt(var + eps), where ``out`` uses that entry's approximate reciprocal
 * square root), and - with a mask - keep [rows,C], one byte per element, 1 where mask != 0.
 *   res, mask (fp32 [rows,C], 0 or 1/(1-p)) may be NULL; keep may be NULL without a mask.
 * Same limits as dfx_add_layernorm_f32 (C % 4 == 0, C <= 1024, 16-byte aligned float buffers; keep 4-byte aligned);
 * every check runs before the launch; rows == 0 returns DFX_OK without one. */
int dfx_add_layernorm_train_f32(const float *x, const float *res, const float *mask, const float *gamma,
                                const float *beta, float *out, float *s, float *mean, float *rstd, unsigned char *keep,
                                long rows, int C, float eps, void *stream);

/* Backward of dfx_add_layernorm_train_f32 from what it left.  With xh = (s - mean) * rstd and g = dy * gamma:
 *   ds[r,:]        = rstd * (g - mean_c(g) - xh * mean_c(g * xh))
 *   grad_res       = ds                                                   [rows,C]
 *   grad_x         = ds without ``keep``; with it ds * scale where keep != 0 and 0 elsewhere (scale = 1/(1-p))
 *   grad_gamma[c]  = sum_r dy * xh,   grad_beta[c] = sum_r dy             [C]
 * Each of the four outputs may be NULL and its work is then skipped; the others are overwritten, never accumulated into
 * (plain stores: the buffers need no zero fill).  Without ``keep`` grad_x and grad_res are the same values: ask for one.
 * No atomics.  The launch has DFX_ADDLN_BWD_GRID(rows) workgroups of four waves - a function of rows alone, no device
 * query; wave w of 4 * grid walks rows w, w + 4 * grid, ... in ascending order with its columns' sums in registers (the
 * terms dy * xh of grad_gamma formed and added in fp64, rounded to fp32 once per wave), the
 * four waves are added in wave order, every workgroup writes row b of ``workspace`` [grid, 2C] (caller-owned, needed for
 * grad_gamma / grad_beta only), and a second launch adds the rows: 16 contiguous slices, each in ascending order, then
 * the slices in ascending order.  Two calls give the same bits, on any device.
 * Checks as the forward, before any launch; rows == 0 launches nothing and zero-fills grad_gamma / grad_beta. */
#define DFX_ADDLN_BWD_ROWS_PER_BLOCK 16
#define DFX_ADDLN_BWD_MAX_GRID 1024
#define DFX_ADDLN_BWD_GRID(rows) \
    (((rows) + DFX_ADDLN_BWD_ROWS_PER_BLOCK - 1) / DFX_ADDLN_BWD_ROWS_PER_BLOCK < DFX_ADDLN_BWD_MAX_GRID \
         ? ((rows) + DFX_ADDLN_BWD_ROWS_PER_BLOCK - 1) / DFX_ADDLN_BWD_ROWS_PER_BLOCK : DFX_ADDLN_BWD_MAX_GRID)
int dfx_add_layernorm_backward_f32(const float *dy, const float *s, const float *mean, const float *rstd,
                                   const float *gamma, const unsigned char *keep, float scale, float *grad_x,
                                   float *grad_res, float *grad_gamma, float *grad_beta, float *workspace,
                                   long rows, int C, void *stream);

/* Box refinement of the iterative decoders and detection heads in one pass:
 *   out[r,c] = sigmoid(delta[r,c] + inverse_sigmoid(ref[r,c]))  for c < ref_dim,  sigmoid(delta[r,c]) otherwise,
 * inverse_sigmoid(x) = log(max(clamp(x,0,1), eps) / max(1 - clamp(x,0,1), eps))
 * (/root/reference/util/misc.py inverse_sigmoid; deformable_transformer_single.py:724-735,
 * deformable_detr_single.py:203-212).  delta, out [rows,4]; ref [rows,ref_dim], ref_dim 2 or 4. */
int dfx_box_refine_f32(const float *delta, const float *ref, int ref_dim, float *out, long rows, float eps,
                       void *stream);

/* nn.GroupNorm(groups, C) of the detector's input projections (Conv1x1 + GroupNorm(32, 256),
 * /root/reference/models/deformable_detr_single.py:101-125,143-150): biased variance over each group's C/groups
 * channels x HW pixels, eps inside the sqrt, per-channel affine.
 *   x [N,C,HW] NCHW;  stats [N*groups*2] scratch (mean, rstd), caller-owned
 *   y: tokens_out = 0 -> [N,C,HW];  tokens_out = 1 -> [N,HW,C]  (the layout the transformer flattens to, so the
 *      reference's separate flatten(2).transpose(1,2) copy is not needed) */
int dfx_group_norm_f32(const float *x, const float *gamma, const float *beta, float *stats, float *y,
                       int N, int C, long HW, int groups, float eps, int tokens_out, void *stream);

/* Backward of dfx_group_norm_f32 (csrc/groupnorm_backward.hip), what autograd computes for the nn.GroupNorm of the input
 * projections when they train.  With xh = (x - mean) * rstd from the forward's ``stats``, m = (C/groups) * HW,
 * a_g = sum_{c in g, p} gamma[c] dy and b_g = sum_{c in g, p} gamma[c] dy xh:
 *   dx[n,c,p]  = rstd * (gamma[c] * dy - a_g / m - xh * b_g / m)      [N,C,HW]
 *   dgamma[c]  = sum_{n,p} dy * xh                                    [C]
 *   dbeta[c]   = sum_{n,p} dy                                         [C]
 * Each of the three outputs may be NULL and is then not computed; the others are overwritten, never accumulated into.
 *   dy: dy_tokens = 0 -> [N,C,HW];  dy_tokens = 1 -> [N,HW,C], the layout of the forward's tokens_out result
 *   x [N,C,HW], stats [N*groups*2] as the forward left them, gamma [C]
 *   workspace: N * C * 2 * DFX_GN_BWD_CHUNKS floats, caller-owned (per-image, per-channel partial sums)
 * No atomics; partial sums are added in ascending pixel-chunk, channel and image order: two calls give the same bits.
 * Argument checks as dfx_group_norm_f32; N * HW == 0 returns DFX_OK without a launch. */
#define DFX_GN_BWD_CHUNKS 16
int dfx_group_norm_backward_f32(const float *dy, const float *x, const float *stats, const float *gamma,
                                float *dx, float *dgamma, float *dbeta, float *workspace,
                                int N, int C, long HW, int groups, int dy_tokens, void *stream);

/* nn.BatchNorm2d in training mode (batch statistics), optionally followed by the exact GELU, of the DFormer depth stem
 * (csrc/batchnorm_train.hip; the reference runs nn.BatchNorm2d and nn.GELU op by op, models/dformer_backbone.py):
 *   mean[c], var[c]  over the N * HW values of channel c, var biased (divided by N * HW)
 *   y = act(gamma[c] * (x - mean[c]) * rstd[c] + beta[c]),  rstd = 1 / sqrt(var + eps),  act DFX_ACT_NONE or DFX_ACT_GELU
 *   stats [2C]: mean[0..C), rstd[C..2C) - what the backward reads
 *   running_mean / running_var [C] (each may be NULL): r = (1 - momentum) * r + momentum * stat (formed in fp64 from the merged
 *     statistics, rounded once), with the UNBIASED variance
 *     (divided by N * HW - 1) for running_var, as nn.BatchNorm2d does; num_batches_tracked is the caller's
 *   x, y [N,C,HW] packed NCHW (y may be NULL: statistics only); gamma, beta [C]
 *   workspace: 6 * C * N * DFX_BN_CHUNKS(HW) floats (used as doubles: 8-byte aligned), caller-owned
 * Every (image, channel) plane is cut into chunks of DFX_BN_CHUNK_PIXELS pixels, one workgroup each - the grid is a function
 * of the shape alone.  A chunk is read once into registers: its mean relative to its first pixel, then its centred second
 * moment, summed in fp64 (never E[x^2] - E[x]^2: the variance survives |mean| >> std); one thread per channel merges the
 * chunks' (count, mean, M2) in ascending (image, chunk) order (Chan et al.), in fp64; mean and rstd are rounded to fp32
 * once.  Accesses are 16 bytes wide when HW % 4 == 0 and x, y are 16-byte aligned, else 4.  No atomics: two calls give the
 * same bits.  Three launches (two without y).
 * Every check runs before the first launch: dimensions positive, N * HW >= 2 (as torch: more than one value per channel),
 * N, C <= 65535, HW < 2^31 - DFX_BN_CHUNK_PIXELS, eps >= 0, 0 <= momentum <= 1. */
#define DFX_BN_CHUNK_PIXELS 8192
#define DFX_BN_CHUNKS(HW) (((HW) + DFX_BN_CHUNK_PIXELS - 1) / DFX_BN_CHUNK_PIXELS)
int dfx_batch_norm_train_f32(const float *x, const float *gamma, const float *beta, float *running_mean,
                             float *running_var, float *y, float *stats, float *workspace, int N, int C, long HW,
                             double eps, double momentum, int act, void *stream);

/* Backward of dfx_batch_norm_train_f32 from x and the ``stats`` it left (and the forward's eps); neither the BatchNorm output nor
 * the GELU output is needed.  With xh = (x - mean) * rstd, z = gamma * xh + beta and g = dy (act none) or dy * gelu'(z)
 * (DFX_ACT_GELU, z as the forward formed it from ``stats``), m = N * HW:
 *   dx        = gamma * rstd * (g - sum g / m - xh * sum (g xh) / m)    [N,C,HW]
 *   dgamma[c] = sum g * xh,   dbeta[c] = sum g                           [C]
 * Each of the three outputs may be NULL and its work is then skipped (all NULL: DFX_OK without a launch); the others are
 * overwritten with plain stores, never accumulated into.  workspace: 8 * C * N * DFX_BN_CHUNKS(HW) floats (used as doubles:
 * 8-byte aligned), caller-owned.
 * Two launches: per group of DFX_BN_BWD_GROUP(P) consecutive chunks (the forward's chunks, P = N * DFX_BN_CHUNKS(HW) per channel
 * in (image, chunk) order; at most DFX_BN_BWD_MAX_GROUPS groups per channel) the fp64 sums of g, g u, u and u^2 with
 * u = x - mean[c], then - per workgroup of one chunk - the channel's group sums added by one wave (lane l adds groups l and
 * l + 64 in ascending order, then a shuffle butterfly),
 * the batch statistics formed from them again in fp64 (dx does not inherit the rounding of ``stats`` to fp32: with few values
 * per channel the three terms of dx cancel to eps / var of their size) and the chunk's dx in one pass, rounded to fp32 once.
 * No atomics, the same bits every call.  Checks as the forward, before any launch. */
#define DFX_BN_BWD_MAX_GROUPS 128
#define DFX_BN_BWD_GROUP(P) (((P) + DFX_BN_BWD_MAX_GROUPS - 1) / DFX_BN_BWD_MAX_GROUPS)
int dfx_batch_norm_backward_f32(const float *dy, const float *x, const float *stats, const float *gamma,
                                const float *beta, float *dx, float *dgamma, float *dbeta, float *workspace, int N,
                                int C, long HW, double eps, int act, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_FUSED_H */
