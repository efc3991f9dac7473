// nn.BatchNorm2d with batch statistics (training mode), optionally followed by the exact GELU, forward and backward, as
// streaming kernels (include/dfx_fused.h, dfx_batch_norm_train_f32 / dfx_batch_norm_backward_f32).  The depth stem runs it on
// 16 channels of 400 x 667 pixels per frame: a workgroup per channel cannot fill the chip, so every (channel, image) plane is
// cut into chunks of DFX_BN_CHUNK_PIXELS pixels and a workgroup of 256 threads owns one chunk, 32 pixels per thread.
//   forward   1. stats: the chunk is read ONCE into registers.  Its first pixel k is the pivot: x - k, formed in fp64, is exact,
//                so a channel with |mean| >> std loses nothing in the sum; d = sum (x - k) / count, then the centred second
//                moment m2 = sum (x - k - d)^2 from the same registers, both sums in fp64.  (k, d, m2) go to the workspace.
//             2. finalize: one thread per channel merges its chunks in ascending (image, chunk) order with Chan's update of
//                (count, mean, M2), in fp64; writes stats = (mean[C], rstd[C]) and updates the running buffers.
//             3. apply: y = act(gamma * rstd * (x - mean) + beta), one pass.
//   backward  1. sums: per group of chunks (at most 128 groups per channel), in fp64, sum g, sum g u, sum u, sum u^2 with u = x - mean and g = dy (* gelu'(z), z recomputed
//                from x as the forward formed it), to the workspace.
//             2. apply: a wave adds the channel's group sums (lane l takes groups l, l + 64, in ascending order, then one
//                shuffle butterfly), forms the statistics again in fp64, then dx = gamma * rstd * (g - mean(g) - xh * mean(g xh))
//                in one pass (fp64 per element, rounded once); the workgroup of the channel's first chunk writes dgamma, dbeta.
// Every access is 16 bytes wide when H*W is a multiple of 4 and the pointers are 16-byte aligned, else one float.
// No atomics; every sum has a fixed order that depends on the shape alone: two calls give the same bits.  Every output
// element is written by exactly one thread, none is read.  HBM-bound: the forward reads x twice (the second time from
// L2 / Infinity Cache where the map fits) and writes y; the backward reads x and dy twice and writes dx.
#include "dfx_common.h"
#include "dfx_conv.h"
#include "dfx_fused.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 32;
constexpr int kChunk = DFX_BN_CHUNK_PIXELS;
static_assert(kChunk == kThreads * kPerThread, "a chunk is 32 pixels per thread of one workgroup");

template <int W>
__device__ __forceinline__ void ld(const float *p, float (&v)[W])
{
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = p[0];
    }
}

template <int W>
__device__ __forceinline__ void st(float *p, const float (&v)[W])
{
    if constexpr (W == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

using dfx::wave_sum;

// the four waves' sums added in wave order; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    v = wave_sum(v);
    __syncthreads();                                            // (sh may still be read from the call before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// the exact GELU, as activate() of mfma_tile.h states it: behind one shared function either the convolutions' code or
// bn_apply's comes out different (profiles/r19_kernel_twins.txt), so the line stands twice
__device__ __forceinline__ float gelu(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752440f)); }

// d/dz of the exact GELU: Phi(z) + z * phi(z)
__device__ __forceinline__ float gelu_grad(float z)
{
    return 0.5f * (1.f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

struct Chunk {
    long base;      // offset of the chunk's first pixel in the tensor
    int cnt;        // pixels in it (the last chunk of a plane may be ragged)
    int c;
};

// blockIdx = (chunk, image, channel)
__device__ __forceinline__ Chunk my_chunk(int C, int HW)
{
    const int k = blockIdx.x, n = blockIdx.y, c = blockIdx.z;
    return {((long)n * C + c) * HW + (long)k * kChunk, min(kChunk, HW - k * kChunk), c};
}

// ws (as doubles)[(c * P + n * chunks + k) * 3 ..] = pivot, mean - pivot, centred second moment of the chunk;  P = N * chunks
template <int W>
__global__ __launch_bounds__(kThreads) void bn_stats(const float *__restrict__ x, double *__restrict__ ws, int C, int HW)
{
    __shared__ double sh[4];
    const Chunk ch = my_chunk(C, HW);
    const float *p = x + ch.base;
    const double pivot = (double)p[0];
    float v[kPerThread];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kPerThread / W; ++i) {
        const int e = (i * kThreads + (int)threadIdx.x) * W;
        float q[W];
#pragma unroll
        for (int j = 0; j < W; ++j) q[j] = p[0];
        if (e < ch.cnt) ld<W>(p + e, q);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            v[i * W + j] = q[j];
            s += (double)q[j] - pivot;                          // (exact; 0 for the slots past the chunk's end)
        }
    }
    const double d = block_sum(s, sh) / (double)ch.cnt;
    double m2 = 0.0;
#pragma unroll
    for (int i = 0; i < kPerThread / W; ++i) {
        const int e = (i * kThreads + (int)threadIdx.x) * W;
        if (e < ch.cnt) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const double t = ((double)v[i * W + j] - pivot) - d;
                m2 = fma(t, t, m2);
            }
        }
    }
    m2 = block_sum(m2, sh);
    if (threadIdx.x == 0) {
        const long P = (long)gridDim.y * gridDim.x;
        double *out = ws + ((long)ch.c * P + (long)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        out[0] = pivot, out[1] = d, out[2] = m2;
    }
}

// one thread per channel: Chan's merge of (count, mean, M2) over the chunks in ascending (image, chunk) order
__global__ __launch_bounds__(64) void bn_finalize(const double *__restrict__ ws, float *__restrict__ stats,
                                                  float *__restrict__ running_mean, float *__restrict__ running_var, int N, int C,
                                                  int HW, int chunks, double eps, double momentum)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const long P = (long)N * chunks;
    double cnt = 0.0, mean = 0.0, M2 = 0.0;
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < chunks; ++k) {
            const double *w = ws + ((long)c * P + (long)n * chunks + k) * 3;
            const double nb = (double)min(kChunk, HW - k * kChunk), mb = w[0] + w[1];
            const double delta = mb - mean, tot = cnt + nb;
            mean += delta * (nb / tot);
            M2 += w[2] + delta * delta * (cnt * nb / tot);
            cnt = tot;
        }
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(M2 / cnt + eps));
    // (formed in fp64 and rounded once)
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (M2 / (cnt - 1.0)));
}

template <int W, int ACT>
__global__ __launch_bounds__(kThreads) void bn_apply(const float *__restrict__ x, const float *__restrict__ stats,
                                                     const float *__restrict__ gamma, const float *__restrict__ beta,
                                                     float *__restrict__ y, int C, int HW)
{
    const Chunk ch = my_chunk(C, HW);
    const float mean = stats[ch.c], a = gamma[ch.c] * stats[C + ch.c], b = beta[ch.c];
    const float *p = x + ch.base;
    float *o = y + ch.base;
#pragma unroll 4
    for (int i = 0; i < kPerThread / W; ++i) {
        const int e = (i * kThreads + (int)threadIdx.x) * W;
        if (e < ch.cnt) {
            float q[W];
            ld<W>(p + e, q);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float z = fmaf(q[j] - mean, a, b);
                q[j] = ACT == DFX_ACT_GELU ? gelu(z) : z;
            }
            st<W>(o + e, q);
        }
    }
}

// The backward works on u = x - mean (mean: the forward's fp32 statistic, a pivot next to the true mean; the difference is
// formed in fp64 and exact) and keeps four fp64 sums per channel: sum g, sum g u, sum u, sum u^2.  From them the apply kernel
// forms the batch statistics again in fp64 - dx does not inherit the rounding of ``stats`` to fp32, which a channel with few
// values, where g - mean(g) - xh mean(g xh) cancels to eps / var of its terms, would show in its second digit.  Only the GELU's
// argument is the forward's own fp32 z.
// One workgroup adds a GROUP of ``per`` consecutive chunks of its channel (chunk q = image * chunks + chunk of the image, in
// ascending order; per = DFX_BN_BWD_GROUP(P), so that a channel leaves at most DFX_BN_BWD_MAX_GROUPS partial sums however many
// images there are - the apply kernel's workgroups each add them all again).  blockIdx = (group, 0, channel);
// ws (as doubles)[(c * groups + group) * 4 ..] = the four sums over the group
template <int W, int ACT>
__global__ __launch_bounds__(kThreads) void bn_bwd_sums(const float *__restrict__ dy, const float *__restrict__ x,
                                                        const float *__restrict__ stats, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, double *__restrict__ ws, int C, int HW,
                                                        int chunks, long P, int per)
{
    __shared__ double sh[4];
    const int c = blockIdx.z;
    const float mean = stats[c], a = gamma[c] * stats[C + c], b = beta[c];
    double sg = 0.0, sgu = 0.0, su = 0.0, suu = 0.0;
    const long q0 = (long)blockIdx.x * per, q1 = min(P, q0 + per);
    for (long q = q0; q < q1; ++q) {
        const long n = q / chunks;
        const int k = (int)(q - n * chunks), cnt = min(kChunk, HW - k * kChunk);
        const long base = (n * C + c) * HW + (long)k * kChunk;
        const float *px = x + base, *pg = dy + base;
#pragma unroll 4
        for (int i = 0; i < kPerThread / W; ++i) {
            const int e = (i * kThreads + (int)threadIdx.x) * W;
            if (e < cnt) {
                float v[W], g[W];
                ld<W>(px + e, v);
                ld<W>(pg + e, g);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const double u = (double)v[j] - (double)mean;
                    const double gg = ACT == DFX_ACT_GELU ? (double)(g[j] * gelu_grad(fmaf(v[j] - mean, a, b))) : (double)g[j];
                    sg += gg;
                    sgu = fma(gg, u, sgu);
                    su += u;
                    suu = fma(u, u, suu);
                }
            }
        }
    }
    sg = block_sum(sg, sh), sgu = block_sum(sgu, sh), su = block_sum(su, sh), suu = block_sum(suu, sh);
    if (threadIdx.x == 0) {
        double *out = ws + ((long)c * gridDim.x + blockIdx.x) * 4;
        out[0] = sg, out[1] = sgu, out[2] = su, out[3] = suu;
    }
}

// with dx: blockIdx = (chunk, image, channel); without: one workgroup per channel
template <int W, int ACT>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply(const float *__restrict__ dy, const float *__restrict__ x,
                                                         const float *__restrict__ stats, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const double *__restrict__ ws,
                                                         float *__restrict__ dx, float *__restrict__ dgamma,
                                                         float *__restrict__ dbeta, int C, int HW, int groups, double m, double eps)
{
    __shared__ double k[3];
    const int c = blockIdx.z;
    if (threadIdx.x < 64) {
        const double *w = ws + (long)c * groups * 4;
        double sg = 0.0, sgu = 0.0, su = 0.0, suu = 0.0;
        for (int i = threadIdx.x; i < groups; i += 64) sg += w[i * 4], sgu += w[i * 4 + 1], su += w[i * 4 + 2], suu += w[i * 4 + 3];
        sg = wave_sum(sg), sgu = wave_sum(sgu), su = wave_sum(su), suu = wave_sum(suu);
        if (threadIdx.x == 0) {
            const double mu = su / m;                                   // true mean - pivot
            const double var = fmax(suu / m - mu * mu, 0.0);
            const double rstd = 1.0 / sqrt(var + eps);
            const double cov = sgu - sg * mu;                           // sum g (u - mu)
            const double k2 = rstd * rstd * cov / m;                    // xh mean(g xh) = (u - mu) k2
            k[0] = (double)gamma[c] * rstd, k[1] = sg / m - mu * k2, k[2] = k2;
            if (blockIdx.x == 0 && blockIdx.y == 0) {
                if (dgamma) dgamma[c] = (float)(rstd * cov);
                if (dbeta) dbeta[c] = (float)sg;
            }
        }
    }
    if (!dx) return;
    __syncthreads();
    const Chunk ch = my_chunk(C, HW);
    const float mean = stats[c], a = gamma[c] * stats[C + c], b = beta[c];
    const double ka = k[0], k1 = k[1], k2 = k[2];
    const float *px = x + ch.base, *pg = dy + ch.base;
    float *o = dx + ch.base;
#pragma unroll 4
    for (int i = 0; i < kPerThread / W; ++i) {
        const int e = (i * kThreads + (int)threadIdx.x) * W;
        if (e < ch.cnt) {
            float q[W], g[W];
            ld<W>(px + e, q);
            ld<W>(pg + e, g);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const double u = (double)q[j] - (double)mean;
                const double gg = ACT == DFX_ACT_GELU ? (double)(g[j] * gelu_grad(fmaf(q[j] - mean, a, b))) : (double)g[j];
                q[j] = (float)(ka * (gg - k1 - u * k2));
            }
            st<W>(o + e, q);
        }
    }
}

using dfx::aligned16;

int check_shape(const char *what, int N, int C, long HW, int act)
{
    const char *why = nullptr;
    int rc = DFX_EINVAL;
    if (N <= 0 || C <= 0 || HW <= 0) why = "bad dimension";
    else if (act != DFX_ACT_NONE && act != DFX_ACT_GELU) why = "activation must be DFX_ACT_NONE or DFX_ACT_GELU";
    else if ((long)N * HW < 2) why = "needs more than one value per channel";
    else if (HW >= (1L << 31) - kChunk || N > 65535 || C > 65535 || (long)N * DFX_BN_CHUNKS(HW) >= (1L << 31) / 3)
        why = "too large", rc = DFX_ERANGE;
    if (!why) return DFX_OK;
    return dfx::fail(rc, "%s: %s", what, why);
}

}  // namespace

extern "C" int dfx_batch_norm_train_f32(const float *x, const float *gamma, const float *beta, float *running_mean,
                                        float *running_var, float *y, float *stats, float *workspace, int N, int C, long HW,
                                        double eps, double momentum, int act, void *stream)
{
    int rc = check_shape("batch_norm_train", N, C, HW, act);
    if (rc != DFX_OK) return rc;
    if (!x || !gamma || !beta || !stats || !workspace) return dfx::fail(DFX_EINVAL, "batch_norm_train: null pointer");
    if (!(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return dfx::fail(DFX_EINVAL, "batch_norm_train: eps >= 0 and momentum in [0, 1]");
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return dfx::fail(DFX_EINVAL, "batch_norm_train: the workspace must be 8-byte aligned");
    double *ws = reinterpret_cast<double *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int hw = (int)HW, chunks = (int)DFX_BN_CHUNKS(HW);
    const dim3 grid((unsigned)chunks, (unsigned)N, (unsigned)C);
    const bool vec = hw % 4 == 0 && aligned16(x) && (!y || aligned16(y));
    if (vec) hipLaunchKernelGGL(bn_stats<4>, grid, dim3(kThreads), 0, st, x, ws, C, hw);
    else hipLaunchKernelGGL(bn_stats<1>, grid, dim3(kThreads), 0, st, x, ws, C, hw);
    if ((rc = dfx::check_launch("bn_stats")) != DFX_OK) return rc;
    hipLaunchKernelGGL(bn_finalize, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, ws, stats, running_mean, running_var,
                       N, C, hw, chunks, eps, momentum);
    if ((rc = dfx::check_launch("bn_finalize")) != DFX_OK || !y) return rc;
#define DFX_BN_APPLY(W, ACT) hipLaunchKernelGGL((bn_apply<W, ACT>), grid, dim3(kThreads), 0, st, x, stats, gamma, beta, y, C, hw)
    if (act == DFX_ACT_GELU) { if (vec) DFX_BN_APPLY(4, DFX_ACT_GELU); else DFX_BN_APPLY(1, DFX_ACT_GELU); }
    else { if (vec) DFX_BN_APPLY(4, DFX_ACT_NONE); else DFX_BN_APPLY(1, DFX_ACT_NONE); }
#undef DFX_BN_APPLY
    return dfx::check_launch("bn_apply");
}

extern "C" int dfx_batch_norm_backward_f32(const float *dy, const float *x, const float *stats, const float *gamma,
                                           const float *beta, float *dx, float *dgamma, float *dbeta, float *workspace, int N,
                                           int C, long HW, double eps, int act, void *stream)
{
    int rc = check_shape("batch_norm_backward", N, C, HW, act);
    if (rc != DFX_OK) return rc;
    if (!dx && !dgamma && !dbeta) return DFX_OK;
    if (!dy || !x || !stats || !gamma || !beta || !workspace) return dfx::fail(DFX_EINVAL, "batch_norm_backward: null pointer");
    if (!(eps >= 0.0)) return dfx::fail(DFX_EINVAL, "batch_norm_backward: eps >= 0");
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return dfx::fail(DFX_EINVAL, "batch_norm_backward: the workspace must be 8-byte aligned");
    double *ws = reinterpret_cast<double *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int hw = (int)HW, chunks = (int)DFX_BN_CHUNKS(HW);
    const long P = (long)N * chunks;
    const int per = (int)DFX_BN_BWD_GROUP(P), groups = (int)((P + per - 1) / per);
    const double m = (double)N * (double)HW;
    const dim3 sgrid((unsigned)groups, 1, (unsigned)C);
    const dim3 agrid = dx ? dim3((unsigned)chunks, (unsigned)N, (unsigned)C) : dim3(1, 1, (unsigned)C);
    const bool vec = hw % 4 == 0 && aligned16(x) && aligned16(dy) && (!dx || aligned16(dx));
#define DFX_BN_BWD(W, ACT)                                                                                                      \
    do {                                                                                                                        \
        hipLaunchKernelGGL((bn_bwd_sums<W, ACT>), sgrid, dim3(kThreads), 0, st, dy, x, stats, gamma, beta, ws, C, hw, chunks, P, \
                           per);                                                                                                \
        if ((rc = dfx::check_launch("bn_bwd_sums")) != DFX_OK) return rc;                                                      \
        hipLaunchKernelGGL((bn_bwd_apply<W, ACT>), agrid, dim3(kThreads), 0, st, dy, x, stats, gamma, beta, ws, dx,            \
                           dgamma, dbeta, C, hw, groups, m, eps);                                                                    \
    } while (0)
    if (act == DFX_ACT_GELU) { if (vec) DFX_BN_BWD(4, DFX_ACT_GELU); else DFX_BN_BWD(1, DFX_ACT_GELU); }
    else { if (vec) DFX_BN_BWD(4, DFX_ACT_NONE); else DFX_BN_BWD(1, DFX_ACT_NONE); }
#undef DFX_BN_BWD
    return dfx::check_launch("bn_bwd_apply");
}
