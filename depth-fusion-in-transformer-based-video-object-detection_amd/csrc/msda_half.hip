// Multi-scale deformable attention with a 2-byte value map (bf16 / fp16), forward and backward, for
// gfx950 (MI355X / CDNA4).
//
// The mixed-precision form of the operator in msda_forward.hip / msda_backward.hip: what
// MSDeformAttn hands the op under torch.autocast - value from a Linear (bf16 / fp16), sampling
// locations and attention weights in fp32 (include/dfx_msda.h, dfx_msda_forward_bf16).  Only the
// value map, grad_output and the forward output are 2-byte; the arithmetic is the fp32 op's:
// corner weights, products and the sum over L*P samples in fp32, one rounding per output element
// (a plain conversion, v_cvt_pk_{bf16,f16}_f32).  Backward accumulates grad_value into an fp32
// buffer with float atomics (a packed 2-byte atomic would round at every add).
//
//   forward, M = 8, D = 32, P = 4, L <= 4, 16-byte aligned value / out: msda_half_fwd_taps.  Phase A
//            is msda_fwd_taps' (msda_tap.h, write_taps with 512-byte token rows); phase B gathers
//            each corner as 2-byte channels, accumulates in fp32 registers and stores the output
//            row in the value dtype.  Two gather widths, the same bits:
//              wide    4 lanes x 16 B per head: 8 channels a lane, both queries of the wave in one pass
//              narrow  8 lanes x  8 B per head: 4 channels a lane, one query per pass (the fp32 mapping)
//            wide for L = 1 (bf16, 32 frames: enc 98 us against 130, dec 12.9 against 14.2), narrow for more
//            levels (enc L4: 601 us against 621; wide holds 16 corner rows of 16 B per level in flight and
//            needs 178-256 VGPRs at L >= 2).  DFX_MSDA_HALF_NARROW=1 takes narrow for every L (A/B).
//   forward, anything else: msda_half_fwd_generic, one thread per output element, scalar 2-byte reads
//            (odd D, any alignment).
//   backward, M = 8, D = 32, 16-byte aligned value / grad_out: msda_half_bwd_m8d32 (msda_bwd_m8d32 with
//            8-byte corner and grad_out reads); anything else msda_half_bwd_generic.
//
// Algorithmic bytes of a forward call: 2*N*S*M*D + 12*N*Lq*M*L*P + 2*N*Lq*M*D
// (5.91 MB per encoder frame, S = Lq = 4200, L = 1; 10.21 MB in fp32).
#include <hip/hip_bf16.h>

#include "dfx_common.h"
#include "msda_tap.h"

namespace {

using dfx::fma4;
using dfx::xcd_remap;

// K consecutive 2-byte channels, loaded / stored as one 2K-byte access
template <typename T, int K>
struct alignas(2 * K) Pack {
    T v[K];
};

template <typename T>
__device__ __forceinline__ float4 widen4(const Pack<T, 4> &p)
{
    return make_float4((float)p.v[0], (float)p.v[1], (float)p.v[2], (float)p.v[3]);
}

template <typename T>
__device__ __forceinline__ Pack<T, 4> narrow4(const float4 &a)
{
    Pack<T, 4> p;
    p.v[0] = static_cast<T>(a.x);
    p.v[1] = static_cast<T>(a.y);
    p.v[2] = static_cast<T>(a.z);
    p.v[3] = static_cast<T>(a.w);
    return p;
}

// ---------------------------------------------------------------------------------------------
// Forward fast path: M = 8, D = 32, P = 4, LT levels (1..4), 2-byte value / out, fp32 loc / aw.
// Token rows are 512 bytes (8 heads x 64 B).  A 256-thread workgroup = 4 waves x 2 queries.
// ---------------------------------------------------------------------------------------------
template <int LT, typename T, bool WIDE>
__global__ __launch_bounds__(256) void msda_half_fwd_taps(const T *__restrict__ value,
                                                          const int64_t *__restrict__ shapes,
                                                          const int64_t *__restrict__ lsi,
                                                          const float *__restrict__ loc,
                                                          const float *__restrict__ aw, int NQ, int Lq,
                                                          int S, int iters, T *__restrict__ out)
{
    constexpr int QW = 2;                 // queries per wave per iteration
    constexpr int TAPS = QW * LT * 32;
    __shared__ uint4 s_off[4][TAPS];
    __shared__ float4 s_w[4][TAPS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    uint4 *toff = s_off[wave];
    float4 *tw = s_w[wave];
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned slab = (unsigned)S * 512u;     // bytes of one batch element's value map

    dfx::LevelDims<LT> lv;
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        lv.H[l] = (int)shapes[2 * l];
        lv.W[l] = (int)shapes[2 * l + 1];
        lv.R[l] = (int)lsi[l];
    }

    for (int it = 0; it < iters; ++it) {
        const int q0 = ((blk * iters + it) * 4 + wave) * QW;   // first query of this wave (uniform)
        if (q0 >= NQ) break;
        // ---- phase A: one tap per lane ----
        dfx::write_taps<LT, QW, 512u>(loc, aw, q0, NQ, lane, lv, toff, tw);
        dfx::wave_lds_fence();
        // ---- phase B: gather ----
        const int b0 = q0 / Lq;
        const char *vb = reinterpret_cast<const char *>(value) + (size_t)b0 * slab;
        if (WIDE) {
            // lane = (query qq = lane>>5, head m = (lane>>2)&7, channel octet cg = lane&3); the pair may
            // straddle two batch elements, so the second one's slab goes into the lane's offset
            // (< 2 * slab <= S * 1024 < 2^32: the launcher's bound).  A query past NQ has zero taps.
            const int qq = lane >> 5, m = (lane >> 2) & 7;
            const int qi = q0 + qq;
            const int b = qi < NQ ? qi / Lq : b0;
            const unsigned lane_b = (unsigned)(lane & 3) * 16u + (unsigned)(b - b0) * slab;
            const uint4 *qo = toff + qq * LT * 32;
            const float4 *qw = tw + qq * LT * 32;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                uint4 o[4];
                float4 w[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    o[p] = qo[(l * 4 + p) * 8 + m];
                    w[p] = qw[(l * 4 + p) * 8 + m];
                }
                Pack<T, 8> v[16];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    v[p * 4 + 0] = *reinterpret_cast<const Pack<T, 8> *>(vb + (o[p].x + lane_b));
                    v[p * 4 + 1] = *reinterpret_cast<const Pack<T, 8> *>(vb + (o[p].y + lane_b));
                    v[p * 4 + 2] = *reinterpret_cast<const Pack<T, 8> *>(vb + (o[p].z + lane_b));
                    v[p * 4 + 3] = *reinterpret_cast<const Pack<T, 8> *>(vb + (o[p].w + lane_b));
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float wk[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const Pack<T, 8> &c = v[p * 4 + k];
                        fma4(lo, wk[k], make_float4((float)c.v[0], (float)c.v[1], (float)c.v[2], (float)c.v[3]));
                        fma4(hi, wk[k], make_float4((float)c.v[4], (float)c.v[5], (float)c.v[6], (float)c.v[7]));
                    }
                }
            }
            if (qi < NQ) {
                const Pack<T, 4> a = narrow4<T>(lo), c = narrow4<T>(hi);
                Pack<T, 8> r;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    r.v[k] = a.v[k];
                    r.v[4 + k] = c.v[k];
                }
                *reinterpret_cast<Pack<T, 8> *>(out + (long)qi * 256 + (lane & 31) * 8) = r;
            }
        } else {
            // lane = (head m = lane>>3, channel quad cg = lane&7), one query per pass
            const int m = lane >> 3;
            const unsigned lane_b = (unsigned)(lane & 7) * 8u;
#pragma unroll
            for (int qq = 0; qq < QW; ++qq) {
                const int qi = q0 + qq;
                if (qi < NQ) {
                    const char *vq = reinterpret_cast<const char *>(value) + (size_t)(qi / Lq) * slab;
                    const uint4 *qo = toff + qq * LT * 32;
                    const float4 *qw = tw + qq * LT * 32;
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int l = 0; l < LT; ++l) {
                        uint4 o[4];
                        float4 w[4];
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            o[p] = qo[(l * 4 + p) * 8 + m];
                            w[p] = qw[(l * 4 + p) * 8 + m];
                        }
                        Pack<T, 4> v[16];
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            v[p * 4 + 0] = *reinterpret_cast<const Pack<T, 4> *>(vq + (o[p].x + lane_b));
                            v[p * 4 + 1] = *reinterpret_cast<const Pack<T, 4> *>(vq + (o[p].y + lane_b));
                            v[p * 4 + 2] = *reinterpret_cast<const Pack<T, 4> *>(vq + (o[p].z + lane_b));
                            v[p * 4 + 3] = *reinterpret_cast<const Pack<T, 4> *>(vq + (o[p].w + lane_b));
                        }
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            fma4(acc, w[p].x, widen4<T>(v[p * 4 + 0]));
                            fma4(acc, w[p].y, widen4<T>(v[p * 4 + 1]));
                            fma4(acc, w[p].z, widen4<T>(v[p * 4 + 2]));
                            fma4(acc, w[p].w, widen4<T>(v[p * 4 + 3]));
                        }
                    }
                    *reinterpret_cast<Pack<T, 4> *>(out + (long)qi * 256 + lane * 4) = narrow4<T>(acc);
                }
            }
        }
        dfx::wave_lds_fence();   // the next iteration overwrites the taps
    }
}

// ---------------------------------------------------------------------------------------------
// Forward generic path: any M, D, L, P.  One thread per output element, channel fastest, grid-stride;
// the arithmetic of msda_fwd_generic<float> with 2-byte value reads and one rounding at the store.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void msda_half_fwd_generic(const T *__restrict__ value,
                                                             const int64_t *__restrict__ shapes,
                                                             const int64_t *__restrict__ lsi,
                                                             const float *__restrict__ loc,
                                                             const float *__restrict__ aw, long total, int S,
                                                             int M, int D, int L, int Lq, int P,
                                                             T *__restrict__ out)
{
    const int row = M * D;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        long t = idx;
        const int c = (int)(t % D);
        t /= D;
        const long samp = t;
        const int m = (int)(t % M);
        t /= M;
        const int b = (int)(t / Lq);
        const T *vb = value + (long)b * S * row + m * D + c;
        long wp = samp * L * P, lp = wp * 2;
        float col = 0.f;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const T *vl = vb + (long)((int)lsi[l]) * row;
            for (int p = 0; p < P; ++p, ++wp, lp += 2) {
                const float h_im = loc[lp + 1] * (float)H - 0.5f;
                const float w_im = loc[lp] * (float)W - 0.5f;
                if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
                    const float hf = floorf(h_im), wf = floorf(w_im);
                    const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
                    const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
                    float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
                    if (h0 >= 0 && w0 >= 0) v1 = (float)vl[(long)(h0 * W + w0) * row];
                    if (h0 >= 0 && w1 <= W - 1) v2 = (float)vl[(long)(h0 * W + w1) * row];
                    if (h1 <= H - 1 && w0 >= 0) v3 = (float)vl[(long)(h1 * W + w0) * row];
                    if (h1 <= H - 1 && w1 <= W - 1) v4 = (float)vl[(long)(h1 * W + w1) * row];
                    col += (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4) * aw[wp];
                }
            }
        }
        out[idx] = static_cast<T>(col);
    }
}

__device__ __forceinline__ float head_sum(float v)
{
    // sum over the 8 lanes (lane&7) that share one head
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------
// Backward fast path: M = 8, D = 32, any L and P.  msda_bwd_m8d32 with 8-byte reads of the value
// corners and of grad_out; grad_value (fp32, [N,S,M,D]) takes float atomics.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void msda_half_bwd_m8d32(const T *__restrict__ value,
                                                           const int64_t *__restrict__ shapes,
                                                           const int64_t *__restrict__ lsi,
                                                           const float *__restrict__ loc,
                                                           const float *__restrict__ aw,
                                                           const T *__restrict__ grad_out, int NQ, int Lq, int S,
                                                           int L, int P, float *__restrict__ grad_value,
                                                           float *__restrict__ grad_loc,
                                                           float *__restrict__ grad_aw)
{
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int qi = blk * 4 + (threadIdx.x >> 6);
    if (qi >= NQ) return;                       // whole wave leaves together: shuffles below are safe
    const int m = lane >> 3, cg = lane & 7;
    const int b = qi / Lq;
    const long samp = (long)qi * 8 + m;
    const long chan = (long)b * S * 256 + m * 32 + cg * 4;
    const float4 top = widen4<T>(*reinterpret_cast<const Pack<T, 4> *>(grad_out + (long)qi * 256 + m * 32 + cg * 4));
    long wp = samp * (long)(L * P), lp = wp * 2;

    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const long lvl = chan + (long)((int)lsi[l]) * 256;
        const T *vl = value + lvl;
        float *gl = grad_value + lvl;
        for (int p = 0; p < P; ++p, ++wp, lp += 2) {
            const float weight = aw[wp];
            const float h_im = loc[lp + 1] * (float)H - 0.5f;
            const float w_im = loc[lp] * (float)W - 0.5f;
            float g_w = 0.f, g_h = 0.f, g_a = 0.f;
            // the in-range test depends on (query, head) only: uniform over the 8 lanes of a head
            if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
                const float hf = floorf(h_im), wf = floorf(w_im);
                const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
                const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
                const float tx = top.x * weight, ty = top.y * weight, tz = top.z * weight, tw = top.w * weight;
                float4 gh = make_float4(0.f, 0.f, 0.f, 0.f), gw = gh, val = gh;
#define DFX_CORNER(cond, yy, xx, wgt, GH, GW)                                              \
                if (cond) {                                                                \
                    const int o = ((yy) * W + (xx)) * 256;                                 \
                    const float4 v = widen4<T>(*reinterpret_cast<const Pack<T, 4> *>(vl + o)); \
                    gh.x += (GH) * v.x; gh.y += (GH) * v.y; gh.z += (GH) * v.z; gh.w += (GH) * v.w; \
                    gw.x += (GW) * v.x; gw.y += (GW) * v.y; gw.z += (GW) * v.z; gw.w += (GW) * v.w; \
                    val.x += (wgt) * v.x; val.y += (wgt) * v.y; val.z += (wgt) * v.z; val.w += (wgt) * v.w; \
                    unsafeAtomicAdd(gl + o, (wgt) * tx); unsafeAtomicAdd(gl + o + 1, (wgt) * ty);    \
                    unsafeAtomicAdd(gl + o + 2, (wgt) * tz); unsafeAtomicAdd(gl + o + 3, (wgt) * tw);\
                }
                DFX_CORNER(h0 >= 0 && w0 >= 0, h0, w0, hh * hw, -hw, -hh)
                DFX_CORNER(h0 >= 0 && w1 <= W - 1, h0, w1, hh * lw, -lw, hh)
                DFX_CORNER(h1 <= H - 1 && w0 >= 0, h1, w0, lh * hw, hw, -lh)
                DFX_CORNER(h1 <= H - 1 && w1 <= W - 1, h1, w1, lh * lw, lw, lh)
#undef DFX_CORNER
                g_a = top.x * val.x + top.y * val.y + top.z * val.z + top.w * val.w;
                g_w = (float)W * (gw.x * tx + gw.y * ty + gw.z * tz + gw.w * tw);
                g_h = (float)H * (gh.x * tx + gh.y * ty + gh.z * tz + gh.w * tw);
            }
            g_w = head_sum(g_w);
            g_h = head_sum(g_h);
            g_a = head_sum(g_a);
            if (cg == 0) {
                unsafeAtomicAdd(grad_loc + lp, g_w);
                unsafeAtomicAdd(grad_loc + lp + 1, g_h);
                unsafeAtomicAdd(grad_aw + wp, g_a);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Backward generic path: any M, D, L, P; msda_bwd_generic<float> with 2-byte value / grad_out reads.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void msda_half_bwd_generic(const T *__restrict__ value,
                                                             const int64_t *__restrict__ shapes,
                                                             const int64_t *__restrict__ lsi,
                                                             const float *__restrict__ loc,
                                                             const float *__restrict__ aw,
                                                             const T *__restrict__ grad_out, long total, int S,
                                                             int M, int D, int L, int Lq, int P,
                                                             float *__restrict__ grad_value,
                                                             float *__restrict__ grad_loc,
                                                             float *__restrict__ grad_aw)
{
    const int row = M * D;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        long t = idx;
        const int c = (int)(t % D);
        t /= D;
        const long samp = t;
        const int m = (int)(t % M);
        t /= M;
        const int b = (int)(t / Lq);
        const long chan = (long)b * S * row + m * D + c;
        const float top = (float)grad_out[idx];
        long wp = samp * L * P, lp = wp * 2;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const long lvl = chan + (long)((int)lsi[l]) * row;
            const T *vl = value + lvl;
            float *gl = grad_value + lvl;
            for (int p = 0; p < P; ++p, ++wp, lp += 2) {
                const float weight = aw[wp];
                const float h_im = loc[lp + 1] * (float)H - 0.5f;
                const float w_im = loc[lp] * (float)W - 0.5f;
                if (!(h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W)) continue;
                const float hf = floorf(h_im), wf = floorf(w_im);
                const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
                const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
                const float tg = top * weight;
                float gh = 0.f, gw = 0.f, val = 0.f;
                if (h0 >= 0 && w0 >= 0) {
                    const long o = (long)(h0 * W + w0) * row;
                    const float v = (float)vl[o];
                    gh -= hw * v; gw -= hh * v; val += hh * hw * v;
                    unsafeAtomicAdd(gl + o, hh * hw * tg);
                }
                if (h0 >= 0 && w1 <= W - 1) {
                    const long o = (long)(h0 * W + w1) * row;
                    const float v = (float)vl[o];
                    gh -= lw * v; gw += hh * v; val += hh * lw * v;
                    unsafeAtomicAdd(gl + o, hh * lw * tg);
                }
                if (h1 <= H - 1 && w0 >= 0) {
                    const long o = (long)(h1 * W + w0) * row;
                    const float v = (float)vl[o];
                    gh += hw * v; gw -= lh * v; val += lh * hw * v;
                    unsafeAtomicAdd(gl + o, lh * hw * tg);
                }
                if (h1 <= H - 1 && w1 <= W - 1) {
                    const long o = (long)(h1 * W + w1) * row;
                    const float v = (float)vl[o];
                    gh += lw * v; gw += lh * v; val += lh * lw * v;
                    unsafeAtomicAdd(gl + o, lh * lw * tg);
                }
                unsafeAtomicAdd(grad_aw + wp, top * val);
                unsafeAtomicAdd(grad_loc + lp, (float)W * gw * tg);
                unsafeAtomicAdd(grad_loc + lp + 1, (float)H * gh * tg);
            }
        }
    }
}

template <typename T>
int forward_half(const T *value, const int64_t *shapes, const int64_t *lsi, const float *loc, const float *aw,
                 int N, int S, int M, int D, int L, int Lq, int P, T *out, void *stream)
{
    // an empty value map (S = 0) may come as a null pointer: nothing of it is read
    const int rc = dfx::check_dims(S == 0 ? static_cast<const void *>(out) : value, shapes, lsi, loc, aw, out, N, S,
                                   M, D, L, Lq, P);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long nq = (long)N * Lq;
    if (S == 0 || L == 0 || P == 0) {   // nothing to sample: the reference returns zeros
        if (hipMemsetAsync(out, 0, sizeof(T) * nq * M * D, st) != hipSuccess)
            return dfx::fail(DFX_ELAUNCH, "msda forward (2-byte value): memset failed");
        return DFX_OK;
    }
    // S * 1024 < 2^32 keeps a tap offset plus a second batch element's slab (wide gather) in 32 bits
    if (M == 8 && D == 32 && P == 4 && L <= 4 && nq < (1L << 28) && (long)S * 1024 < (1L << 32) &&
        dfx::aligned16(value) && dfx::aligned16(out) && (reinterpret_cast<uintptr_t>(loc) & 7u) == 0) {
        int iters = 1;
        while (iters < 8 && nq / (8L * iters * 2) >= 2048) iters *= 2;
        const int grid = (int)((nq + 8L * iters - 1) / (8L * iters));
        const bool wide = L == 1 && !dfx::tuning().msda_half_narrow;
#define DFX_LAUNCH(LT)                                                                                      \
        if (wide)                                                                                           \
            hipLaunchKernelGGL((msda_half_fwd_taps<LT, T, true>), dim3(grid), dim3(256), 0, st, value, shapes, \
                               lsi, loc, aw, (int)nq, Lq, S, iters, out);                                   \
        else                                                                                                \
            hipLaunchKernelGGL((msda_half_fwd_taps<LT, T, false>), dim3(grid), dim3(256), 0, st, value, shapes, \
                               lsi, loc, aw, (int)nq, Lq, S, iters, out)
        switch (L) {
            case 1: DFX_LAUNCH(1); break;
            case 2: DFX_LAUNCH(2); break;
            case 3: DFX_LAUNCH(3); break;
            default: DFX_LAUNCH(4); break;
        }
#undef DFX_LAUNCH
        return dfx::check_launch("msda_half_fwd_taps");
    }
    const long total = nq * M * D;
    hipLaunchKernelGGL((msda_half_fwd_generic<T>), dim3(dfx::grid_for(total)), dim3(256), 0, st, value, shapes, lsi,
                       loc, aw, total, S, M, D, L, Lq, P, out);
    return dfx::check_launch("msda_half_fwd_generic");
}

template <typename T>
int backward_half(const T *value, const int64_t *shapes, const int64_t *lsi, const float *loc, const float *aw,
                  const T *grad_out, int N, int S, int M, int D, int L, int Lq, int P, float *grad_value,
                  float *grad_loc, float *grad_aw, void *stream)
{
    const int rc = dfx::check_dims(S == 0 ? static_cast<const void *>(grad_out) : value, shapes, lsi, loc, aw,
                                   grad_out, N, S, M, D, L, Lq, P);
    if (rc < 0) return rc;
    if (rc == 1 || S == 0 || L == 0 || P == 0) return DFX_OK;   // S = 0: every sample falls outside, all gradients 0
    if (!grad_value || !grad_loc || !grad_aw) return dfx::fail(DFX_EINVAL, "msda backward: null gradient buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long nq = (long)N * Lq;
    if (M == 8 && D == 32 && nq < (1L << 29) && dfx::aligned16(value) && dfx::aligned16(grad_out)) {
        hipLaunchKernelGGL((msda_half_bwd_m8d32<T>), dim3((int)((nq + 3) / 4)), dim3(256), 0, st, value, shapes, lsi,
                           loc, aw, grad_out, (int)nq, Lq, S, L, P, grad_value, grad_loc, grad_aw);
        return dfx::check_launch("msda_half_bwd_m8d32");
    }
    const long total = nq * M * D;
    hipLaunchKernelGGL((msda_half_bwd_generic<T>), dim3(dfx::grid_for(total)), dim3(256), 0, st, value, shapes, lsi,
                       loc, aw, grad_out, total, S, M, D, L, Lq, P, grad_value, grad_loc, grad_aw);
    return dfx::check_launch("msda_half_bwd_generic");
}

template <typename T>
const T *as(const uint16_t *p)
{
    return reinterpret_cast<const T *>(p);
}

}  // namespace

extern "C" int dfx_msda_forward_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                     const float *loc, const float *aw, int N, int S, int M, int D, int L, int Lq,
                                     int P, uint16_t *out, void *stream)
{
    return forward_half<__hip_bfloat16>(as<__hip_bfloat16>(value), shapes, lsi, loc, aw, N, S, M, D, L, Lq, P,
                                        reinterpret_cast<__hip_bfloat16 *>(out), stream);
}

extern "C" int dfx_msda_forward_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                    const float *loc, const float *aw, int N, int S, int M, int D, int L, int Lq,
                                    int P, uint16_t *out, void *stream)
{
    return forward_half<_Float16>(as<_Float16>(value), shapes, lsi, loc, aw, N, S, M, D, L, Lq, P,
                                  reinterpret_cast<_Float16 *>(out), stream);
}

extern "C" int dfx_msda_backward_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                      const float *loc, const float *aw, const uint16_t *grad_out, int N, int S,
                                      int M, int D, int L, int Lq, int P, float *grad_value_f32, float *grad_loc,
                                      float *grad_aw, void *stream)
{
    return backward_half<__hip_bfloat16>(as<__hip_bfloat16>(value), shapes, lsi, loc, aw,
                                         as<__hip_bfloat16>(grad_out), N, S, M, D, L, Lq, P, grad_value_f32,
                                         grad_loc, grad_aw, stream);
}

extern "C" int dfx_msda_backward_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                     const float *loc, const float *aw, const uint16_t *grad_out, int N, int S,
                                     int M, int D, int L, int Lq, int P, float *grad_value_f32, float *grad_loc,
                                     float *grad_aw, void *stream)
{
    return backward_half<_Float16>(as<_Float16>(value), shapes, lsi, loc, aw, as<_Float16>(grad_out), N, S, M, D,
                                   L, Lq, P, grad_value_f32, grad_loc, grad_aw, stream);
}
