// Optimizer step (include/dfx_optim.h): the total gradient norm, norm clipping and AdamW of all parameters of a model as
// streaming passes over a chunk table - one launch for the norm, one for the update.
//
// The work is bandwidth: the update reads p, g, m, v and writes p, m, v (28 B per element), the norm reads g (4 B).  A
// workgroup of 256 threads takes chunk records grid-striding; inside a chunk thread t handles the 16-byte vectors t,
// t + 256, ... (or, for a tensor with a misaligned pointer, the elements t, t + 256, ...), so a wave always touches one
// contiguous 1 KiB run per array.  No LDS but the four doubles of the norm's block sums, no atomics, plain vector
// stores.  The per-tensor scalars come from the tensor record (uniform per chunk: scalar loads).
#include "dfx_common.h"
#include "dfx_optim.h"

static_assert(sizeof(dfx_optim_tensor) == 72 && sizeof(dfx_optim_chunk) == 16, "table records as dfx/optim.py packs them");
static_assert(DFX_OPTIM_CHUNK > 0 && DFX_OPTIM_CHUNK % 4 == 0, "a chunk keeps the 16-byte alignment of its tensor");

namespace {

using dfx::fail;
using dfx::wave_sum;

constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;        // 8 workgroups per CU of an MI355X: the memory-bound grid cap

__device__ __forceinline__ bool aligned16_dev(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// elements of the chunk that starts at `first` in a tensor of `numel`
__device__ __forceinline__ int chunk_len(long long numel, long long first)
{
    const long long left = numel - first;
    return left < (long long)DFX_OPTIM_CHUNK ? (left > 0 ? (int)left : 0) : DFX_OPTIM_CHUNK;
}

// ---- norm -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    v = wave_sum(v);
    __syncthreads();                                            // (sh may still be read from the chunk before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(const dfx_optim_tensor *__restrict__ tensors,
                                                               const dfx_optim_chunk *__restrict__ chunks, int n_chunks,
                                                               double *__restrict__ partials)
{
    __shared__ double sh[4];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const dfx_optim_chunk ch = chunks[c];
        const dfx_optim_tensor *t = tensors + ch.tensor;
        const int len = chunk_len(t->numel, ch.first);
        const float *g = t->grad + ch.first;
        double s = 0.0;
        if (aligned16_dev(g)) {
            const float4 *g4 = reinterpret_cast<const float4 *>(g);
            const int n4 = len >> 2;
            for (int i = threadIdx.x; i < n4; i += kThreads) {
                const float4 q = g4[i];
                s += (double)q.x * (double)q.x;
                s += (double)q.y * (double)q.y;
                s += (double)q.z * (double)q.z;
                s += (double)q.w * (double)q.w;
            }
            const int i = (n4 << 2) + threadIdx.x;              // the tail: at most 3 elements
            if (i < len) s += (double)g[i] * (double)g[i];
        } else {
            for (int i = threadIdx.x; i < len; i += kThreads) s += (double)g[i] * (double)g[i];
        }
        s = block_sum(s, sh);
        if (threadIdx.x == 0) partials[c] = s;
    }
}

// Sum of partials[0 .. n) by the whole workgroup: thread t adds partials t, t + 256, ... in index order (eight loads in flight
// at a time - a chain of dependent L2 round trips would hold back every workgroup's first chunk), block_sum adds the 256 sums.
// Every workgroup that calls it gets the same bits.
__device__ __forceinline__ double block_total(const double *__restrict__ partials, int n, double *sh)
{
    double s = 0.0;
    int i = threadIdx.x;
    for (; i + 7 * kThreads < n; i += 8 * kThreads) {
        double a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = partials[i + j * kThreads];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += a[j];
    }
    for (; i < n; i += kThreads) s += partials[i];
    return block_sum(s, sh);
}

__device__ __forceinline__ float norm_of(double sumsq) { return (float)sqrt(sumsq); }

// torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1) in fp32; a NaN stays a NaN as under torch.clamp
__device__ __forceinline__ float clip_coef(float norm, float max_norm)
{
    const float c = max_norm / (norm + 1e-6f);
    return c > 1.f ? 1.f : c;
}

// ---- update ---------------------------------------------------------------------------------------------------------
struct Scalars {
    float coef, decay, w, beta2, omb2, step_size, bc2_sqrt, eps;
};

// torch's order: p.mul_(decay); m.lerp_(g, w); v.mul_(beta2).addcmul_(g, g, value=1-beta2);
// p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(eps), value=-step_size)
__device__ __forceinline__ void adamw_element(float &p, float g, float &m, float &v, const Scalars &k)
{
    g *= k.coef;
    p *= k.decay;
    const float d = g - m;
    m = k.w < 0.5f ? m + k.w * d : g - d * (1.f - k.w);        // at::lerp
    v = k.beta2 * v + k.omb2 * (g * g);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p + (-k.step_size) * (m / denom);
}

__global__ __launch_bounds__(kThreads) void adamw_step_kernel(const dfx_optim_tensor *__restrict__ tensors,
                                                              const dfx_optim_chunk *__restrict__ chunks, int n_chunks,
                                                              const double *__restrict__ partials, float max_norm,
                                                              float *__restrict__ norm_out)
{
    __shared__ double sh[4];
    float coef = 1.f;
    if (partials) {                                             // (uniform over the grid: every thread meets block_sum's barriers)
        const float norm = norm_of(block_total(partials, n_chunks, sh));
        coef = clip_coef(norm, max_norm);
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
    }
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const dfx_optim_chunk ch = chunks[c];
        const dfx_optim_tensor *t = tensors + ch.tensor;
        const Scalars k = {coef, t->decay, t->lerp_weight, t->beta2, t->one_minus_beta2, t->step_size,
                           t->bias_correction2_sqrt, t->eps};
        const int len = chunk_len(t->numel, ch.first);
        float *__restrict__ p = t->param + ch.first;
        const float *__restrict__ g = t->grad + ch.first;
        float *__restrict__ m = t->exp_avg + ch.first;
        float *__restrict__ v = t->exp_avg_sq + ch.first;
        int scalar_from = 0;                                    // first element of the element-by-element part
        if (aligned16_dev(p) && aligned16_dev(g) && aligned16_dev(m) && aligned16_dev(v)) {
            float4 *p4 = reinterpret_cast<float4 *>(p);
            const float4 *g4 = reinterpret_cast<const float4 *>(g);
            float4 *m4 = reinterpret_cast<float4 *>(m);
            float4 *v4 = reinterpret_cast<float4 *>(v);
            const int n4 = len >> 2;
            for (int i = threadIdx.x; i < n4; i += kThreads) {
                float4 pp = p4[i], mm = m4[i], vv = v4[i];
                const float4 gg = g4[i];
                adamw_element(pp.x, gg.x, mm.x, vv.x, k);
                adamw_element(pp.y, gg.y, mm.y, vv.y, k);
                adamw_element(pp.z, gg.z, mm.z, vv.z, k);
                adamw_element(pp.w, gg.w, mm.w, vv.w, k);
                p4[i] = pp, m4[i] = mm, v4[i] = vv;
            }
            scalar_from = n4 << 2;                              // the tail: at most 3 elements
        }
        for (int i = scalar_from + threadIdx.x; i < len; i += kThreads) {
            float pp = p[i], mm = m[i], vv = v[i];
            adamw_element(pp, g[i], mm, vv, k);
            p[i] = pp, m[i] = mm, v[i] = vv;
        }
    }
}

inline int check_tables(const char *what, const void *tensors, const void *chunks, int n_chunks)
{
    if (n_chunks < 0) return fail(DFX_EINVAL, "%s: bad dimension (n_chunks=%d)", what, n_chunks);
    if (n_chunks == 0) return 1;
    if (!tensors || !chunks) return fail(DFX_EINVAL, "%s: null pointer", what);
    return 0;
}

inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int dfx_optim_chunk_elements(void) { return DFX_OPTIM_CHUNK; }

extern "C" int dfx_grad_sqnorm_f32(const dfx_optim_tensor *tensors, const dfx_optim_chunk *chunks, int n_chunks,
                                   double *partials, void *stream)
{
    const int rc = check_tables("grad_sqnorm", tensors, chunks, n_chunks);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    if (!partials) return fail(DFX_EINVAL, "grad_sqnorm: null pointer");
    if (!aligned8(partials)) return fail(DFX_EINVAL, "grad_sqnorm: partials must be 8-byte aligned");
    const int grid = n_chunks < kMaxGrid ? n_chunks : kMaxGrid;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, tensors, chunks, n_chunks, partials);
    return dfx::check_launch("grad_sqnorm");
}

extern "C" int dfx_adamw_step_f32(const dfx_optim_tensor *tensors, const dfx_optim_chunk *chunks, int n_chunks,
                                  const double *partials, float max_norm, float *norm_out, void *stream)
{
    const int rc = check_tables("adamw_step", tensors, chunks, n_chunks);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    if (partials) {
        if (!aligned8(partials)) return fail(DFX_EINVAL, "adamw_step: partials must be 8-byte aligned");
        if (!(max_norm > 0.f)) return fail(DFX_EINVAL, "adamw_step: max_norm must be positive with partials (max_norm=%g)", (double)max_norm);
        if (norm_out && (reinterpret_cast<uintptr_t>(norm_out) & 3u)) return fail(DFX_EINVAL, "adamw_step: norm_out must be 4-byte aligned");
    }
    const int grid = n_chunks < kMaxGrid ? n_chunks : kMaxGrid;
    hipLaunchKernelGGL(adamw_step_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, tensors, chunks, n_chunks,
                       partials, max_norm, norm_out);
    return dfx::check_launch("adamw_step");
}
