// The tail of every transformer sub-layer (gfx950):  out = LayerNorm(residual + dropout(x)).  One forward kernel behind the
// inference entry (dfx_add_layernorm_f32) and the training entry (dfx_add_layernorm_train_f32), and the backward of the
// latter, all on one decomposition: one wave per row, the row in registers (<= 4 float4 per lane), xor-shuffle
// reductions, 16-byte accesses.  HBM-bound; algorithmic bytes per row of
// C floats (DESIGN.md kernel table): training forward 4C * (2 read + 2 written) + 8, with a mask 4C more read and C written;
// backward 4C * (2 read + 1 written) + 8, with a mask C more read and 4C more written.  No atomics anywhere: the
// parameter gradients go through a [grid, 2C] workspace that a second launch adds up in a fixed order.
#include "dfx_common.h"
#include "dfx_fused.h"

namespace {

// x * m rounded to fp32 on its own: the empty asm keeps the compiler from contracting the product into the residual add
// (an fma would not have the bits of the module chain's separate dropout and add kernels)
__device__ __forceinline__ float mul_rounded(float a, float b)
{
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// Forward, both entries: v = res + x (* mask), out = LN(v): mean and variance by two in-register passes (nn.LayerNorm's
// formula: biased variance, eps under the square root).  TRAIN adds what the backward reads: s = v, mean, rstd and (with a
// mask) one keep byte per element; TRAIN = false touches none of mask, s, mean_out, rstd_out and keep.
// The arithmetic of dfx_add_layernorm_f32 and of dfx_add_layernorm_train_f32 is this one source, with contraction off: which
// products are fused into an fma is written out, not left to the compiler (which decides per kernel).  The placement is
// frozen because it is today's bits, those of every trained checkpoint's inference tail:
//   variance, 1 chunk:       (a a + b b) + (c c + d d), no fma
//   variance, 2 or 4 chunks: fma(a, a, b b) + fma(c, c, d d)
//   result:                  fma((v - mean) rstd, gamma, beta)
// tests/test_addln_train_gpu.py's torch.equal between the two entries therefore checks the contract of the C ABI (same
// inputs, same ``out``), not one kernel's transcription of the other.
template <int CHUNKS, bool TRAIN>
__global__ __launch_bounds__(256) void add_layernorm(const float *__restrict__ x, const float *__restrict__ res,
                                                     const float *__restrict__ mask, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, float *__restrict__ out,
                                                     float *__restrict__ s, float *__restrict__ mean_out,
                                                     float *__restrict__ rstd_out, unsigned char *__restrict__ keep,
                                                     long rows, int C, float eps)
{
#pragma clang fp contract(off)
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float4 v[CHUNKS];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const int c = k * 256 + lane * 4;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            v[k] = *reinterpret_cast<const float4 *>(x + row * C + c);
            if (TRAIN && mask) {
                const float4 m = *reinterpret_cast<const float4 *>(mask + row * C + c);
                v[k].x = mul_rounded(v[k].x, m.x); v[k].y = mul_rounded(v[k].y, m.y);
                v[k].z = mul_rounded(v[k].z, m.z); v[k].w = mul_rounded(v[k].w, m.w);
                const unsigned flags = (m.x != 0.f ? 1u : 0u) | (m.y != 0.f ? 1u << 8 : 0u) | (m.z != 0.f ? 1u << 16 : 0u) |
                                       (m.w != 0.f ? 1u << 24 : 0u);
                *reinterpret_cast<unsigned *>(keep + row * C + c) = flags;
            }
            if (res) {
                const float4 r = *reinterpret_cast<const float4 *>(res + row * C + c);
                v[k].x += r.x; v[k].y += r.y; v[k].z += r.z; v[k].w += r.w;
            }
            if (TRAIN) *reinterpret_cast<float4 *>(s + row * C + c) = v[k];
            sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
        }
    }
    // (both butterflies stay open-coded: through dfx::wave_sum the TRAIN instantiations take 2 to 5 more VGPRs)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        if (k * 256 + lane * 4 < C) {
            const float a = v[k].x - mean, b = v[k].y - mean, c2 = v[k].z - mean, d = v[k].w - mean;
            if (CHUNKS == 1) sq += (a * a + b * b) + (c2 * c2 + d * d);
            else sq += __builtin_fmaf(a, a, b * b) + __builtin_fmaf(c2, c2, d * d);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    const float rstd = rsqrtf(sq / (float)C + eps);
    if (TRAIN && lane == 0) {
        // what the backward multiplies every xh by is the correctly rounded 1 / sqrt, not the approximate rsqrtf that
        // ``out`` is made with (up to 1 ulp off, which would be an error of every gradient's row)
        mean_out[row] = mean;
        rstd_out[row] = 1.0f / sqrtf(sq / (float)C + eps);
    }
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const int c = k * 256 + lane * 4;
        if (c < C) {
            const float4 g = *reinterpret_cast<const float4 *>(gamma + c);
            const float4 b = *reinterpret_cast<const float4 *>(beta + c);
            float4 o;
            o.x = __builtin_fmaf((v[k].x - mean) * rstd, g.x, b.x);
            o.y = __builtin_fmaf((v[k].y - mean) * rstd, g.y, b.y);
            o.z = __builtin_fmaf((v[k].z - mean) * rstd, g.z, b.z);
            o.w = __builtin_fmaf((v[k].w - mean) * rstd, g.w, b.w);
            *reinterpret_cast<float4 *>(out + row * C + c) = o;
        }
    }
}

// what both forward entries do once their arguments have passed: one wave per row, 4 rows per workgroup
template <bool TRAIN>
int launch_forward(const char *what, const float *x, const float *res, const float *mask, const float *gamma,
                   const float *beta, float *out, float *s, float *mean, float *rstd, unsigned char *keep, long rows, int C,
                   float eps, void *stream)
{
    if ((rows + 3) / 4 >= (1L << 31)) return dfx::fail(DFX_ERANGE, "%s: too many rows", what);
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int chunks = (C + 255) / 256;
#define DFX_GO(CH) \
    hipLaunchKernelGGL((add_layernorm<CH, TRAIN>), grid, block, 0, st, x, res, mask, gamma, beta, out, s, mean, rstd, keep, rows, C, eps)
    if (chunks == 1) DFX_GO(1);
    else if (chunks == 2) DFX_GO(2);
    else DFX_GO(4);
#undef DFX_GO
    return dfx::check_launch(what);
}

// Backward.  Wave w of workgroup b is wave b * 4 + w of 4 * gridDim.x; it walks rows w, w + waves, w + 2 waves, ... in
// that (ascending) order, the next row's dy and s in flight while this row is worked on.  Per row, with
// xh = (s - mean) rstd and g = dy gamma:  ds = rstd (g - mean_c(g) - xh mean_c(g xh)).
// DS: grad_x / grad_res are wanted;  PARAMS: sum_rows dy xh and sum_rows dy are kept per lane column and leave as one
// workspace row per workgroup, the four waves added in wave order.
template <int CHUNKS, bool DS, bool PARAMS>
__global__ __launch_bounds__(256) void add_layernorm_backward(const float *__restrict__ dy, const float *__restrict__ s,
                                                              const float *__restrict__ mean, const float *__restrict__ rstd,
                                                              const float *__restrict__ gamma,
                                                              const unsigned char *__restrict__ keep, float scale,
                                                              float *__restrict__ grad_x, float *__restrict__ grad_res,
                                                              float *__restrict__ workspace, long rows, int C)
{
    __shared__ float4 part[PARAMS ? 4 * 2 * CHUNKS * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * 4;
    // sum_rows dy xh: each term (dy (s - mean) rstd) is formed and added in fp64, as the library's CPU kernel forms it - in
    // fp32 the roundings of s - mean and of the product by rstd are the whole error of a short sum (1 row: 1.0e-7 of the
    // largest element against 1.7e-8).  A handful of fp64 operations per element, far below the memory time.
    double dgam[CHUNKS][4];
    float4 gam[CHUNKS], dbet[CHUNKS];
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const int c = k * 256 + lane * 4;
        gam[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (DS && c < C) gam[k] = *reinterpret_cast<const float4 *>(gamma + c);
        dgam[k][0] = dgam[k][1] = dgam[k][2] = dgam[k][3] = 0.0;
        dbet[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 ndy[CHUNKS], ns[CHUNKS];
    float nmean = 0.f, nrstd = 0.f;
    long row = (long)blockIdx.x * 4 + wave;
    auto fetch = [&](long r) {
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k) {
            const int c = k * 256 + lane * 4;
            if (c < C) {
                ndy[k] = *reinterpret_cast<const float4 *>(dy + r * C + c);
                ns[k] = *reinterpret_cast<const float4 *>(s + r * C + c);
            }
        }
        nmean = mean[r];
        nrstd = rstd[r];
    };
    if (row < rows) fetch(row);
    for (; row < rows; row += waves) {
        float4 d[CHUNKS], xh[CHUNKS], sv[CHUNKS];
        const float mu = nmean, rs = nrstd;
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k) {
            d[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            sv[k] = make_float4(mu, mu, mu, mu);
            if (k * 256 + lane * 4 < C) {
                d[k] = ndy[k];
                sv[k] = ns[k];
                xh[k] = make_float4((ns[k].x - mu) * rs, (ns[k].y - mu) * rs, (ns[k].z - mu) * rs, (ns[k].w - mu) * rs);
            }
        }
        if (row + waves < rows) fetch(row + waves);
        if (PARAMS) {
#pragma unroll
            for (int k = 0; k < CHUNKS; ++k) {
                const double m = (double)mu, r = (double)rs;
                dgam[k][0] += (double)d[k].x * (((double)sv[k].x - m) * r);
                dgam[k][1] += (double)d[k].y * (((double)sv[k].y - m) * r);
                dgam[k][2] += (double)d[k].z * (((double)sv[k].z - m) * r);
                dgam[k][3] += (double)d[k].w * (((double)sv[k].w - m) * r);
                dbet[k].x += d[k].x; dbet[k].y += d[k].y; dbet[k].z += d[k].z; dbet[k].w += d[k].w;
            }
        }
        if (DS) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int k = 0; k < CHUNKS; ++k) {       // (lanes past C hold zeros)
                d[k].x *= gam[k].x; d[k].y *= gam[k].y; d[k].z *= gam[k].z; d[k].w *= gam[k].w;
                a += (d[k].x + d[k].y) + (d[k].z + d[k].w);
                b += (d[k].x * xh[k].x + d[k].y * xh[k].y) + (d[k].z * xh[k].z + d[k].w * xh[k].w);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
            }
            a /= (float)C;
            b /= (float)C;
#pragma unroll
            for (int k = 0; k < CHUNKS; ++k) {
                const int c = k * 256 + lane * 4;
                if (c < C) {
                    float4 o;
                    o.x = rs * (d[k].x - a - xh[k].x * b);
                    o.y = rs * (d[k].y - a - xh[k].y * b);
                    o.z = rs * (d[k].z - a - xh[k].z * b);
                    o.w = rs * (d[k].w - a - xh[k].w * b);
                    if (grad_res) *reinterpret_cast<float4 *>(grad_res + row * C + c) = o;
                    if (grad_x) {
                        if (keep) {      // d(x * mask): scale where the element was kept, nothing where it was dropped
                            const unsigned f = *reinterpret_cast<const unsigned *>(keep + row * C + c);
                            o.x = (f & 0xffu) ? o.x * scale : 0.f;
                            o.y = (f & 0xff00u) ? o.y * scale : 0.f;
                            o.z = (f & 0xff0000u) ? o.z * scale : 0.f;
                            o.w = (f & 0xff000000u) ? o.w * scale : 0.f;
                        }
                        *reinterpret_cast<float4 *>(grad_x + row * C + c) = o;
                    }
                }
            }
        }
    }
    if (PARAMS) {
        // part[wave][gamma | beta][chunk][lane]; every wave writes (zeros when it had no row), so nothing is read unwritten
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k) {
            part[((wave * 2 + 0) * CHUNKS + k) * 64 + lane] = make_float4((float)dgam[k][0], (float)dgam[k][1], (float)dgam[k][2], (float)dgam[k][3]);
            part[((wave * 2 + 1) * CHUNKS + k) * 64 + lane] = dbet[k];
        }
        __syncthreads();
        float *dst = workspace + (long)blockIdx.x * 2 * C;
        for (int i = threadIdx.x; i < 2 * CHUNKS * 64; i += 256) {
            const int half = i / (CHUNKS * 64), c = (i - half * CHUNKS * 64) * 4;      // c = chunk * 256 + lane * 4
            if (c < C) {
                float4 t = part[i];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const float4 u = part[w * 2 * CHUNKS * 64 + i];
                    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
                }
                *reinterpret_cast<float4 *>(dst + half * C + c) = t;
            }
        }
    }
}

// The second launch: grad_gamma = sum over the workspace rows of columns [0, C), grad_beta of [C, 2C).  A workgroup owns
// 64 columns; its 16 waves each add one contiguous slice of ceil(grid / 16) rows in ascending order, and the slices are
// added in ascending order.  The order depends on grid and C alone: the same bits on every call and on every device.
constexpr int kReduceSlices = 16;

__global__ __launch_bounds__(1024) void add_layernorm_param_sum(const float *__restrict__ workspace, int grid, int C,
                                                                float *__restrict__ grad_gamma, float *__restrict__ grad_beta)
{
    __shared__ float part[kReduceSlices][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int per = (grid + kReduceSlices - 1) / kReduceSlices;
    const int lo = slice * per, hi = min(grid, lo + per);
    float acc = 0.f;
    if (col < 2 * C) {
#pragma unroll 8
        for (int r = lo; r < hi; ++r) acc += workspace[(long)r * 2 * C + col];
    }
    part[slice][lane] = acc;
    __syncthreads();
    if (slice == 0 && col < 2 * C) {
        float t = part[0][lane];
#pragma unroll
        for (int j = 1; j < kReduceSlices; ++j) t += part[j][lane];
        if (col < C) {
            if (grad_gamma) grad_gamma[col] = t;
        } else if (grad_beta) {
            grad_beta[col - C] = t;
        }
    }
}

template <int CHUNKS>
void launch_backward(bool ds, bool params, dim3 grid, hipStream_t st, const float *dy, const float *s, const float *mean,
                     const float *rstd, const float *gamma, const unsigned char *keep, float scale, float *grad_x,
                     float *grad_res, float *workspace, long rows, int C)
{
#define DFX_GO(DS, PARAMS) \
    hipLaunchKernelGGL((add_layernorm_backward<CHUNKS, DS, PARAMS>), grid, dim3(256), 0, st, dy, s, mean, rstd, gamma, keep, \
                       scale, grad_x, grad_res, workspace, rows, C)
    if (ds && params) DFX_GO(true, true);
    else if (ds) DFX_GO(true, false);
    else DFX_GO(false, true);
#undef DFX_GO
}

}  // namespace

extern "C" int dfx_add_layernorm_train_f32(const float *x, const float *res, const float *mask, const float *gamma,
                                           const float *beta, float *out, float *s, float *mean, float *rstd,
                                           unsigned char *keep, long rows, int C, float eps, void *stream)
{
    if (rows < 0 || C <= 0) return dfx::fail(DFX_EINVAL, "add_layernorm_train: bad dimension");
    if ((C & 3) || C > 1024) return dfx::fail(DFX_EINVAL, "add_layernorm_train: C must be a multiple of 4 and <= 1024");
    if (rows == 0) return DFX_OK;
    if (!x || !gamma || !beta || !out || !s || !mean || !rstd || (mask && !keep))
        return dfx::fail(DFX_EINVAL, "add_layernorm_train: null pointer");
    if (!dfx::aligned16(x) || !dfx::aligned16(out) || !dfx::aligned16(s) || !dfx::aligned16(gamma) || !dfx::aligned16(beta) ||
        (res && !dfx::aligned16(res)) || (mask && (!dfx::aligned16(mask) || (reinterpret_cast<uintptr_t>(keep) & 3u))))
        return dfx::fail(DFX_EINVAL, "add_layernorm_train: buffers must be 16-byte aligned (keep: 4-byte)");
    return launch_forward<true>("add_layernorm_train", x, res, mask, gamma, beta, out, s, mean, rstd, keep, rows, C, eps, stream);
}

// the inference tail (include/dfx_fused.h): the same kernel without what only the backward reads
extern "C" int dfx_add_layernorm_f32(const float *x, const float *res, const float *gamma, const float *beta,
                                     float *out, long rows, int C, float eps, void *stream)
{
    if (rows < 0 || C <= 0) return dfx::fail(DFX_EINVAL, "add_layernorm: bad dimension");
    if (rows == 0) return DFX_OK;
    if (!x || !gamma || !beta || !out) return dfx::fail(DFX_EINVAL, "add_layernorm: null pointer");
    if ((C & 3) || C > 1024 || !dfx::aligned16(x) || !dfx::aligned16(out) || !dfx::aligned16(gamma) ||
        !dfx::aligned16(beta) || (res && !dfx::aligned16(res)))
        return dfx::fail(DFX_EINVAL, "add_layernorm: C must be a multiple of 4 and <= 1024, buffers 16-byte aligned");
    return launch_forward<false>("add_layernorm", x, res, nullptr, gamma, beta, out, nullptr, nullptr, nullptr, nullptr, rows, C, eps, stream);
}

extern "C" int dfx_add_layernorm_backward_f32(const float *dy, const float *s, const float *mean, const float *rstd,
                                              const float *gamma, const unsigned char *keep, float scale, float *grad_x,
                                              float *grad_res, float *grad_gamma, float *grad_beta, float *workspace,
                                              long rows, int C, void *stream)
{
    if (rows < 0 || C <= 0) return dfx::fail(DFX_EINVAL, "add_layernorm_backward: bad dimension");
    if ((C & 3) || C > 1024) return dfx::fail(DFX_EINVAL, "add_layernorm_backward: C must be a multiple of 4 and <= 1024");
    const bool ds = grad_x || grad_res, params = grad_gamma || grad_beta;
    if (!ds && !params) return DFX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rows == 0) {       // sums over no rows
        if (grad_gamma && hipMemsetAsync(grad_gamma, 0, sizeof(float) * C, st) != hipSuccess)
            return dfx::fail(DFX_ELAUNCH, "add_layernorm_backward: cannot zero grad_gamma");
        if (grad_beta && hipMemsetAsync(grad_beta, 0, sizeof(float) * C, st) != hipSuccess)
            return dfx::fail(DFX_ELAUNCH, "add_layernorm_backward: cannot zero grad_beta");
        return DFX_OK;
    }
    if (!dy || !s || !mean || !rstd || (ds && !gamma) || (params && !workspace))
        return dfx::fail(DFX_EINVAL, "add_layernorm_backward: null pointer");
    if (!dfx::aligned16(dy) || !dfx::aligned16(s) || (ds && !dfx::aligned16(gamma)) || (grad_x && !dfx::aligned16(grad_x)) ||
        (grad_res && !dfx::aligned16(grad_res)) || (params && !dfx::aligned16(workspace)) ||
        (keep && (reinterpret_cast<uintptr_t>(keep) & 3u)))
        return dfx::fail(DFX_EINVAL, "add_layernorm_backward: buffers must be 16-byte aligned (keep: 4-byte)");
    const int grid = (int)DFX_ADDLN_BWD_GRID(rows);
    const int chunks = (C + 255) / 256;
    if (chunks == 1) launch_backward<1>(ds, params, dim3(grid), st, dy, s, mean, rstd, gamma, keep, scale, grad_x, grad_res, workspace, rows, C);
    else if (chunks == 2) launch_backward<2>(ds, params, dim3(grid), st, dy, s, mean, rstd, gamma, keep, scale, grad_x, grad_res, workspace, rows, C);
    else launch_backward<4>(ds, params, dim3(grid), st, dy, s, mean, rstd, gamma, keep, scale, grad_x, grad_res, workspace, rows, C);
    int rc = dfx::check_launch("add_layernorm_backward");
    if (rc != DFX_OK || !params) return rc;
    hipLaunchKernelGGL(add_layernorm_param_sum, dim3((2 * C + 63) / 64), dim3(1024), 0, st, workspace, grid, C, grad_gamma, grad_beta);
    return dfx::check_launch("add_layernorm_param_sum");
}
