// Backward of the input projections' GroupNorm (csrc/groupnorm.hip is the forward) as two streaming kernels
// (include/dfx_fused.h, dfx_group_norm_backward_f32).  With xh = (x - mean) * rstd of the forward's stats, m = (C/G) * HW,
// a_g = sum_{c in g, p} gamma_c dy and b_g = sum_{c in g, p} gamma_c dy xh:
//   dx = rstd * (gamma * dy - a_g / m - xh * b_g / m),   dgamma[c] = sum_{n,p} dy xh,   dbeta[c] = sum_{n,p} dy
//   1. sums: one workgroup per (image, 64 channels, pixel chunk) walks its chunk in tiles of 64 x 64 and leaves the
//      per-channel sums of dy and dy * xh of that chunk in the workspace: a lane adds its pixels in ascending order, the
//      64 lanes of a wave meet in a shuffle butterfly (a wave owns a channel: no exchange between waves)
//   2. apply: one workgroup per 64 x 64 tile, as the forward's.  Its first 64 threads add the chunk sums in ascending
//      chunk order, the channels of a group in ascending channel order, and - one workgroup per channel tile - the
//      images in ascending image order for dgamma / dbeta; then the tile is one pass.
// dy comes NCHW or token-major [N, H*W, C] (what flows back into the forward's tokens_out view): token-major tiles are read
// along the channels and cross a 64 x 65 LDS tile, so every global access runs along the fastest dimension of its tensor.
// No atomics, every sum in a fixed order: two calls give the same bits; every output element is written, none read.
// HBM-bound: reads x and dy twice (second read from L2 / Infinity Cache) and stats / gamma / the workspace (a few KB),
// writes dx once and the workspace, dgamma, dbeta.
#include "dfx_common.h"
#include "dfx_fused.h"

namespace {

constexpr int kChunks = DFX_GN_BWD_CHUNKS;

using dfx::wave_sum;

// ws[((n * chunks + chunk) * C + c) * 2] = sum over the chunk's pixels of dy, [.. + 1] = of dy * xh
template <bool TOKENS>
__global__ __launch_bounds__(256) void gn_bwd_sums(const float *__restrict__ dy, const float *__restrict__ x,
                                                   const float *__restrict__ stats, float *__restrict__ ws, int C, int HW,
                                                   int cg, int chunk_px)
{
    __shared__ float tile[64][65];
    __shared__ float mean[64], rstd[64];
    const int n = blockIdx.z, c0 = blockIdx.y * 64, chunk = blockIdx.x;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const float *xn = x + (long)n * C * HW, *dyn = dy + (long)n * C * HW;
    if (threadIdx.x < 64) {
        const int c = min(c0 + (int)threadIdx.x, C - 1);
        const float *st = stats + ((long)n * (C / cg) + c / cg) * 2;
        mean[threadIdx.x] = st[0], rstd[threadIdx.x] = st[1];
    }
    __syncthreads();
    float s1[16], s2[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s1[i] = s2[i] = 0.f;
    const int pbeg = chunk * chunk_px, pend = min(HW, pbeg + chunk_px);
    for (int p0 = pbeg; p0 < pend; p0 += 64) {
        if (TOKENS) {
            __syncthreads();                                         // (the tile before this one has been read)
#pragma unroll 4
            for (int r = ty; r < 64; r += 4) {
                const int p = p0 + r, c = c0 + tx;
                tile[r][tx] = (p < pend && c < C) ? dyn[(long)p * C + c] : 0.f;
            }
            __syncthreads();
        }
        const int p = p0 + tx;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = ty + 4 * i, c = c0 + r;
            if (c < C && p < pend) {
                const float g = TOKENS ? tile[tx][r] : dyn[(long)c * HW + p];
                const float xh = (xn[(long)c * HW + p] - mean[r]) * rstd[r];
                s1[i] += g;
                s2[i] += g * xh;
            }
        }
    }
    float *out = ws + ((long)n * gridDim.x + chunk) * C * 2;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float a = wave_sum(s1[i]), b = wave_sum(s2[i]);
        const int c = c0 + ty + 4 * i;
        if (tx == 0 && c < C) out[c * 2L] = a, out[c * 2L + 1] = b;
    }
}

// channel c of image n: its sums over all pixels, the chunks added in ascending order
__device__ __forceinline__ void channel_sums(const float *ws, int n, int chunks, int C, int c, float &s1, float &s2)
{
    s1 = s2 = 0.f;
    for (int k = 0; k < chunks; ++k) {
        const float *w = ws + (((long)n * chunks + k) * C + c) * 2;
        s1 += w[0], s2 += w[1];
    }
}

// tile = 64 channels x 64 pixels of image blockIdx.z; dx may be NULL (the grid is then one workgroup per channel tile)
template <bool TOKENS>
__global__ __launch_bounds__(256) void gn_bwd_apply(const float *__restrict__ dy, const float *__restrict__ x,
                                                    const float *__restrict__ stats, const float *__restrict__ gamma,
                                                    const float *__restrict__ ws, float *__restrict__ dx,
                                                    float *__restrict__ dgamma, float *__restrict__ dbeta, int N, int C, int HW,
                                                    int cg, int chunks)
{
    __shared__ float tile[64][65];
    __shared__ float mean[64], rstd[64], scale[64], am[64], bm[64];
    const int n = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
        const int c = c0 + threadIdx.x;
        if ((dgamma || dbeta) && blockIdx.x == 0 && n == 0) {
            float dg = 0.f, db = 0.f;
            for (int i = 0; i < N; ++i) {                             // ascending image order
                float s1, s2;
                channel_sums(ws, i, chunks, C, c, s1, s2);
                db += s1, dg += s2;
            }
            if (dgamma) dgamma[c] = dg;
            if (dbeta) dbeta[c] = db;
        }
        if (dx) {
            const int g = c / cg;
            float a = 0.f, b = 0.f;
            for (int cc = g * cg; cc < (g + 1) * cg; ++cc) {
                float s1, s2;
                channel_sums(ws, n, chunks, C, cc, s1, s2);
                a += gamma[cc] * s1, b += gamma[cc] * s2;
            }
            const float *st = stats + ((long)n * (C / cg) + g) * 2;
            const float inv_m = 1.f / ((float)cg * (float)HW);
            mean[threadIdx.x] = st[0], rstd[threadIdx.x] = st[1], scale[threadIdx.x] = gamma[c];
            am[threadIdx.x] = a * inv_m, bm[threadIdx.x] = b * inv_m;
        }
    }
    if (!dx) return;
    const float *xn = x + (long)n * C * HW, *dyn = dy + (long)n * C * HW;
    float *dxn = dx + (long)n * C * HW;
    if (TOKENS) {
#pragma unroll 4
        for (int r = ty; r < 64; r += 4) {
            const int p = p0 + r, c = c0 + tx;
            tile[r][tx] = (p < HW && c < C) ? dyn[(long)p * C + c] : 0.f;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, p = p0 + tx;
        if (c < C && p < HW) {
            const float g = TOKENS ? tile[tx][r] : dyn[(long)c * HW + p];
            const float xh = (xn[(long)c * HW + p] - mean[r]) * rstd[r];
            dxn[(long)c * HW + p] = rstd[r] * (scale[r] * g - am[r] - xh * bm[r]);
        }
    }
}

}  // namespace

extern "C" int dfx_group_norm_backward_f32(const float *dy, const float *x, const float *stats, const float *gamma,
                                           float *dx, float *dgamma, float *dbeta, float *workspace, int N, int C, long HW,
                                           int groups, int dy_tokens, void *stream)
{
    if (N < 0 || C <= 0 || HW < 0 || groups <= 0 || C % groups) return dfx::fail(DFX_EINVAL, "group_norm_backward: bad dimension");
    if ((long)N * HW == 0 || (!dx && !dgamma && !dbeta)) return DFX_OK;
    if (!dy || !x || !stats || !gamma || !workspace) return dfx::fail(DFX_EINVAL, "group_norm_backward: null pointer");
    if (HW >= (1L << 31) || (long)N * groups >= (1L << 31) || N > 65535 || (long)C * kChunks * 2 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "group_norm_backward: too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cg = C / groups, hw = (int)HW;
    const int ptiles = (hw + 63) / 64, ctiles = (C + 63) / 64;
    // at most kChunks pixel chunks of whole 64-pixel tiles per (image, channel tile), none empty
    const int chunk_tiles = (ptiles + kChunks - 1) / kChunks, chunks = (ptiles + chunk_tiles - 1) / chunk_tiles;
    const dim3 sgrid((unsigned)chunks, (unsigned)ctiles, (unsigned)N);
    if (dy_tokens) hipLaunchKernelGGL(gn_bwd_sums<true>, sgrid, dim3(256), 0, st, dy, x, stats, workspace, C, hw, cg, chunk_tiles * 64);
    else hipLaunchKernelGGL(gn_bwd_sums<false>, sgrid, dim3(256), 0, st, dy, x, stats, workspace, C, hw, cg, chunk_tiles * 64);
    int rc = dfx::check_launch("gn_bwd_sums");
    if (rc != DFX_OK) return rc;
    const dim3 grid(dx ? (unsigned)ptiles : 1u, (unsigned)ctiles, dx ? (unsigned)N : 1u);
    if (dy_tokens) hipLaunchKernelGGL(gn_bwd_apply<true>, grid, dim3(256), 0, st, dy, x, stats, gamma, workspace, dx, dgamma, dbeta, N, C, hw, cg, chunks);
    else hipLaunchKernelGGL(gn_bwd_apply<false>, grid, dim3(256), 0, st, dy, x, stats, gamma, workspace, dx, dgamma, dbeta, N, C, hw, cg, chunks);
    return dfx::check_launch("gn_bwd_apply");
}
