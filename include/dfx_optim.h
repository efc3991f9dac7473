/*
 * dfx_optim.h -- C ABI of the optimizer step: total gradient norm, norm clipping and AdamW over ALL parameters of a
 * model, one launch each.
 *
 * Restates what the reference's training loop runs after backward (ref engine_single.py:61-67, engine_multi.py:64):
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) followed by torch.optim.AdamW.step(), fp32.
 *
 * Tables, not one launch per tensor.  The caller describes the step by two arrays in DEVICE memory:
 *   dfx_optim_tensor tensors[]   one record per parameter that has a gradient: its four arrays, its element count and
 *                                the scalars of THIS step, which the host computes in double from that parameter's own
 *                                step count exactly as torch.optim.adamw does and rounds to fp32 once (torch hands the
 *                                same doubles to fp32 kernels, which round them the same way)
 *   dfx_optim_chunk  chunks[]    one record per DFX_OPTIM_CHUNK elements of a tensor, tensor after tensor: the tensor's
 *                                index and the chunk's first element (a multiple of DFX_OPTIM_CHUNK); the last chunk of
 *                                a tensor may be short; a tensor of 0 elements has no chunk
 * Workgroups of 256 threads grid-stride over the chunk records (grid = min(n_chunks, 2048)).  A tensor whose pointers
 * are all 16-byte aligned moves as 16-byte vectors with a scalar tail; any other (a parameter that is a view at an odd
 * offset) element by element.
 *
 * Same conventions as dfx_msda.h: device pointers, caller-owned buffers, enqueue-only on `stream`, no allocation and no
 * synchronisation inside (graph-capturable), 0 / negative return code, text by dfx_last_error().  No atomics: every sum
 * is taken in an order fixed by the tables alone, so a call gives the same bits every time.
 * Additions to the ABI: dfx_abi_version() stays.
 */
#ifndef DFX_OPTIM_H
#define DFX_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

/* elements per chunk record (what one workgroup handles before it takes its next record).  Measured at 2048 .. 65536
 * (profiles/r20_optim_step.txt): 4096 .. 16384 lie within 4 % of each other, 8192 is the fastest norm + update on the
 * large parameter set and within 3 % of the fastest on the small one; 65536 leaves most of the 2048 workgroups idle on
 * a 1.2e7-element model (1.5x slower), 2048 pays for its 4e4 partials (5 % slower on 8e7 elements).  -DDFX_OPTIM_CHUNK=n
 * builds another size (a multiple of 4) for such a measurement. */
#ifndef DFX_OPTIM_CHUNK
#define DFX_OPTIM_CHUNK 8192
#endif

typedef struct dfx_optim_tensor {
    float *param;               /* updated in place */
    const float *grad;          /* read only: the clipped gradient is never written back */
    float *exp_avg;             /* updated in place */
    float *exp_avg_sq;          /* updated in place */
    long long numel;
    float decay;                /* 1 - lr * weight_decay */
    float lerp_weight;          /* 1 - beta1 */
    float beta2;
    float one_minus_beta2;      /* 1 - beta2 */
    float step_size;            /* lr / (1 - beta1^step) */
    float bias_correction2_sqrt; /* sqrt(1 - beta2^step) */
    float eps;
    float reserved;             /* 0 */
} dfx_optim_tensor;             /* 72 bytes */

typedef struct dfx_optim_chunk {
    long long first;            /* first element of the chunk inside its tensor */
    int tensor;                 /* index into tensors[] */
    int reserved;               /* 0 */
} dfx_optim_chunk;              /* 16 bytes */

/* the DFX_OPTIM_CHUNK this library was compiled with (the host builds the chunk table with it) */
int dfx_optim_chunk_elements(void);

/* partials[c] = sum over the elements of chunk c of grad^2, c = 0 .. n_chunks-1: squares and sums in fp64.  Thread t of
 * the workgroup adds its elements in index order, the 256 thread sums are added by a fixed tree.  Only `grad` and `numel`
 * of a tensor record are read.  `partials` is 8-byte aligned. */
int dfx_grad_sqnorm_f32(const dfx_optim_tensor *tensors, const dfx_optim_chunk *chunks, int n_chunks, double *partials,
                        void *stream);

/* One AdamW step of every tensor in the table, per element in fp32 in the operation order of torch's
 * _single_tensor_adamw:
 *     g  = grad * coef                         (only with `partials`)
 *     p *= decay
 *     m += lerp_weight * (g - m)               (torch's lerp: its other form, g - (g - m) * (1 - w), for w >= 0.5)
 *     v  = beta2 * v + one_minus_beta2 * (g * g)
 *     p += -step_size * (m / (sqrt(v) / bias_correction2_sqrt + eps))
 * with correctly rounded square root and division.
 * partials != NULL: the n_chunks sums of dfx_grad_sqnorm_f32 on the same tables (8-byte aligned), max_norm > 0:
 *     norm = (float) sqrt(sum of partials)     (fp64; thread t adds partials t, t + 256, ... in index order, the 256
 *                                              sums are added by the fixed tree of dfx_grad_sqnorm_f32)
 *     coef = min(1, max_norm / (norm + 1e-6f)) (fp32, as torch.nn.utils.clip_grad_norm_; a NaN norm gives a NaN coef)
 * computed on the device by EVERY workgroup of the update launch itself, all with the same bits: no further launch, no
 * host round trip.  (A one-workgroup launch that sums once in front of the update measured 2 - 5 us slower per step:
 * profiles/r20_optim_step.txt.)  `norm` is written to norm_out (may be NULL).
 * partials == NULL: coef is 1, max_norm and norm_out are not looked at. */
int dfx_adamw_step_f32(const dfx_optim_tensor *tensors, const dfx_optim_chunk *chunks, int n_chunks,
                       const double *partials, float max_norm, float *norm_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFX_OPTIM_H */
