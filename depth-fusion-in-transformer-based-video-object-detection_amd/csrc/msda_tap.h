// Sampling "taps" of the wave-per-query MSDA kernels (forward + fused front end), gfx950.
//
// A tap is one (query, head, level, point) sample reduced to what the gather needs:
//   4 byte offsets into the batch element's value slab (level start, corner row and the head's
//   128-byte column already folded in) and 4 bilinear weights already multiplied by the
//   attention weight (0 for corners outside the map and for samples the skip rule drops).
// Taps are computed ONCE per (query, head, point) by one lane - not redundantly by the 8 lanes
// that share a head - staged in LDS in [query][level][point][head] order, and read back by the
// gather phase as two conflict-free 16-byte broadcasts per point.
//
// Also the value-dtype helpers of the MSDA kernels (fp32, fp64, bf16, fp16): the arithmetic type of
// a value dtype and the packed channel loads / stores; and the location arithmetic of the fused front
// end (reference point, location rule), stated once for msda_fused_taps and msda_fused_bwd.
#pragma once
#include <hip/hip_bf16.h>

#include <type_traits>

#include "dfx_common.h"

namespace dfx {

// Arithmetic type of an MSDA kernel with value dtype V: double for fp64, float for fp32, bf16 and fp16
// (a 2-byte value is widened on load; locations, weights and gradients are fp32).
template <typename V>
using Acc = typename std::conditional<std::is_same<V, double>::value, double, float>::type;

// K consecutive channels of a value dtype T, loaded / stored as one access of K * sizeof(T) bytes
template <typename T, int K>
struct alignas(sizeof(T) * K) Pack {
    T v[K];
};

// widen4 / narrow4: 4 channels to and from the fp32 the kernels compute in (the identity for T = float)
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

struct Tap {
    uint4 off;    // byte offsets of the corners (y0,x0) (y0,x1) (y1,x0) (y1,x1)
    float4 w;     // matching weights
};

// Geometry of one sample; follows /root/reference/models/ops/src/cuda/ms_deform_im2col_cuda.cuh
// :281-291 (pixel coordinates, skip rule) and :33-84 (corner validity, bilinear weights).
// `head_bytes` = m * ROW_BYTES / 8, `level_row` = level_start_index[l] (token rows of ROW_BYTES:
// 1 KiB = 8 heads x 32 fp32, 512 B = 8 heads x 32 bf16 / fp16).
template <unsigned ROW_BYTES = 1024u>
__device__ __forceinline__ Tap make_tap(float lx, float ly, float a, int H, int W, int level_row,
                                        int head_bytes)
{
    const float h_im = ly * (float)H - 0.5f;
    const float w_im = lx * (float)W - 0.5f;
    const bool inr = (h_im > -1.f) && (w_im > -1.f) && (h_im < (float)H) && (w_im < (float)W);
    // clamp in float first: keeps the float->int conversion defined for NaN / huge inputs
    const float hf = floorf(fminf(fmaxf(h_im, -1.f), (float)H));
    const float wf = floorf(fminf(fmaxf(w_im, -1.f), (float)W));
    const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
    const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
    const bool top = inr && h0 >= 0, bot = inr && h1 <= H - 1, lef = w0 >= 0, rig = w1 <= W - 1;
    Tap t;
    if (H <= 0 || W <= 0) {
        t.off = make_uint4(0u, 0u, 0u, 0u);
        t.w = make_float4(0.f, 0.f, 0.f, 0.f);
        return t;
    }
    t.w.x = (top && lef) ? hh * hw * a : 0.f;
    t.w.y = (top && rig) ? hh * lw * a : 0.f;
    t.w.z = (bot && lef) ? lh * hw * a : 0.f;
    t.w.w = (bot && rig) ? lh * lw * a : 0.f;
    // clamped, always-in-bounds addresses (an empty level, H or W == 0, never gets here: callers
    // give it zero weights and offset 0)
    const int y0 = max(min(h0, H - 1), 0), y1 = max(min(h1, H - 1), 0);
    const int x0 = max(min(w0, W - 1), 0), x1 = max(min(w1, W - 1), 0);
    const int r0 = level_row + y0 * W, r1 = level_row + y1 * W;
    t.off.x = (unsigned)(r0 + x0) * ROW_BYTES + (unsigned)head_bytes;
    t.off.y = (unsigned)(r0 + x1) * ROW_BYTES + (unsigned)head_bytes;
    t.off.z = (unsigned)(r1 + x0) * ROW_BYTES + (unsigned)head_bytes;
    t.off.w = (unsigned)(r1 + x1) * ROW_BYTES + (unsigned)head_bytes;
    return t;
}

// ---- phase A bookkeeping of the taps kernels (msda_fwd_taps, msda_fused_taps) -----------------
// M = 8 heads, P = 4 points, LT levels; a wave stages the taps of QW queries per iteration, lane (+ 64 c) =
// slot s = ((qq*LT + l)*4 + p)*8 + head of LDS.
template <int LT>
struct LevelDims {
    int H[LT], W[LT], R[LT];     // (H_l, W_l, level_start_index[l]) of every level, filled by the kernel
};

template <int LT>
struct Slot {
    int hm, p, l, qq;            // head, point, level, query of the wave
    __device__ __forceinline__ explicit Slot(int s)
    {
        const int ql = s >> 5;
        hm = s & 7;
        p = (s >> 3) & 3;
        l = (LT == 1) ? 0 : ql % LT;
        qq = (LT == 1) ? ql : ql / LT;
    }
};

// Grid of a taps launch: 8 queries per workgroup and iteration; `iters` doubles (up to 8) while that
// still leaves >= 2048 workgroups
struct TapsGrid {
    int iters;
    unsigned blocks;
};
inline TapsGrid taps_grid(long nq)
{
    int iters = 1;
    while (iters < 8 && nq / (8L * iters * 2) >= 2048) iters *= 2;
    return {iters, (unsigned)((nq + 8L * iters - 1) / (8L * iters))};
}

// Phase A of the unfused forward: the lane reads its (x, y) pair and attention weight once and
// writes its tap.  Queries at or past NQ get zero taps (offset 0, weight 0).
template <int LT, int QW, unsigned ROW_BYTES>
__device__ __forceinline__ void write_taps(const float *__restrict__ loc, const float *__restrict__ aw, int q0,
                                           int NQ, int lane, const LevelDims<LT> lv, uint4 *toff, float4 *tw)
{
    constexpr int TAPS = QW * LT * 32;    // taps per wave per iteration (multiple of 64)
#pragma unroll
    for (int c = 0; c < TAPS / 64; ++c) {
        const int s = c * 64 + lane;
        const Slot<LT> sl(s);
        const int hm = sl.hm, p = sl.p, l = sl.l, qi = q0 + sl.qq;
        Tap t;
        if (qi < NQ) {
            const long e = (((long)qi * 8 + hm) * LT + l) * 4 + p;
            const float2 xy = *reinterpret_cast<const float2 *>(loc + e * 2);
            int H = lv.H[0], W = lv.W[0], R = lv.R[0];
#pragma unroll
            for (int k = 1; k < LT; ++k)
                if (l == k) { H = lv.H[k]; W = lv.W[k]; R = lv.R[k]; }
            t = make_tap<ROW_BYTES>(xy.x, xy.y, aw[e], H, W, R, hm * (int)(ROW_BYTES / 8));
        } else {
            t.off = make_uint4(0u, 0u, 0u, 0u);
            t.w = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        toff[s] = t.off;
        tw[s] = t.w;
    }
}

// ---- the fused front end's location arithmetic (msda_fused_taps; msda_fused_bwd calls the same routines) ----
// Reference point of one (query, level): (x, y) and, for ref_dim 4, the box (w, h) that scales the offsets
struct RefPoint {
    float x, y, kx, ky;
};
template <int REFDIM>
__device__ __forceinline__ RefPoint load_ref(const float *__restrict__ rp)
{
    if constexpr (REFDIM == 2) {
        return {rp[0], rp[1], 0.f, 0.f};
    } else {
        const float4 rr = *reinterpret_cast<const float4 *>(rp);
        return {rr.x, rr.y, rr.z, rr.w};
    }
}

// Sampling location of one point from its offset (ox, oy) on a W x H level (ms_deform_attn.py:102-110):
//   ref_dim 2: ref + off / (W, H)          ref_dim 4: ref_xy + off / P * ref_wh * 0.5   (P = 4)
template <int REFDIM>
__device__ __forceinline__ float2 sample_location(const RefPoint &r, float ox, float oy, int W, int H)
{
    if (REFDIM == 2) return make_float2(r.x + ox / (float)W, r.y + oy / (float)H);
    return make_float2(r.x + ox / 4.f * r.kx * 0.5f, r.y + oy / 4.f * r.ky * 0.5f);
}

// ---- reductions of the (head m = lane >> 3, channel quad cg = lane & 7) lane map (msda_bwd_m8d32, msda_fused_bwd) ----
__device__ __forceinline__ float head_sum(float v)
{
    // sum over the 8 lanes (lane&7) that share one head
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

__device__ __forceinline__ float all_heads_sum(float v)
{
    // v is uniform over the 8 lanes of a head: sum over the 8 heads of the wave
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ void fma4(float4 &acc, float w, const float4 &v)
{
    acc.x = fmaf(w, v.x, acc.x);
    acc.y = fmaf(w, v.y, acc.y);
    acc.z = fmaf(w, v.z, acc.z);
    acc.w = fmaf(w, v.w, acc.w);
}

// Orders a wave's own LDS writes before its own later LDS reads (other lanes' data).  The LDS
// executes one wave's instructions in order, so this only has to stop the compiler from moving
// accesses across it.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Gather phase for ONE query: lane = (head m = lane&7 ... see callers), reads its head's taps of
// every (level, point) from LDS and accumulates 4 channels.
//   vb        : wave-uniform pointer to the batch element's value slab (value dtype V)
//   lane_b    : cg * 4 * sizeof(V) (byte offset of this lane's channel quad inside the head's 32 channels)
//   toff/tw   : LDS tap arrays of this query, [LT][4 points][8 heads]
template <int LT, typename V>
__device__ __forceinline__ float4 gather_query(const char *__restrict__ vb, unsigned lane_b, int m,
                                               const uint4 *toff, const float4 *tw)
{
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        uint4 o[4];
        float4 w[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            o[p] = toff[(l * 4 + p) * 8 + m];
            w[p] = tw[(l * 4 + p) * 8 + m];
        }
        Pack<V, 4> v[16];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            v[p * 4 + 0] = *reinterpret_cast<const Pack<V, 4> *>(vb + (o[p].x + lane_b));
            v[p * 4 + 1] = *reinterpret_cast<const Pack<V, 4> *>(vb + (o[p].y + lane_b));
            v[p * 4 + 2] = *reinterpret_cast<const Pack<V, 4> *>(vb + (o[p].z + lane_b));
            v[p * 4 + 3] = *reinterpret_cast<const Pack<V, 4> *>(vb + (o[p].w + lane_b));
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            fma4(acc, w[p].x, widen4<V>(v[p * 4 + 0]));
            fma4(acc, w[p].y, widen4<V>(v[p * 4 + 1]));
            fma4(acc, w[p].z, widen4<V>(v[p * 4 + 2]));
            fma4(acc, w[p].w, widen4<V>(v[p * 4 + 3]));
        }
    }
    return acc;
}

// ---- host side of the two fused entry points (msda_fused.hip, msda_fused_backward.hip) ----
// What dfx_msda_fused_forward_f32 and dfx_msda_fused_backward_f32 both check (same return values as check_dims).
// `what` heads the error texts, `unfused` is the entry point that takes the geometries the fused kernels do not;
// `rows` is the [N*Lq, 256] operand next to value: out in the forward, grad_out in the backward.
inline int check_fused(const char *what, const char *unfused, const float *value, const int64_t *shapes, const int64_t *lsi,
                       const float *ref, int ref_dim, const float *off, long off_stride, const float *logits,
                       long logit_stride, const float *rows, int N, int S, int M, int D, int L, int Lq, int P)
{
    const int rc = check_dims(value, shapes, lsi, off, logits, rows, N, S, M, D, L, Lq, P);
    if (rc != 0) return rc;
    if (!ref) return fail(DFX_EINVAL, "%s: null reference points", what);
    if (ref_dim != 2 && ref_dim != 4) return fail(DFX_EINVAL, "%s: ref_dim must be 2 or 4, got %d", what, ref_dim);
    if (M != 8 || D != 32 || P != 4 || L < 1 || L > 4)
        return fail(DFX_EINVAL, "msda fused: only M=8, D=32, P=4, 1<=L<=4 is fused (got M=%d D=%d P=%d L=%d); use %s",
                    M, D, P, L, unfused);
    if (off_stride < (long)M * L * P * 2 || logit_stride < (long)M * L * P || ((off_stride | logit_stride) & 3))
        return fail(DFX_EINVAL, "%s: bad row strides", what);
    if (!aligned16(value) || !aligned16(rows) || !aligned16(off) || !aligned16(logits) || (ref_dim == 4 && !aligned16(ref)))
        return fail(DFX_EINVAL, "%s: buffers must be 16-byte aligned", what);
    if ((long)N * Lq >= (1L << 28) || (long)S * 1024 >= (1L << 32)) return fail(DFX_ERANGE, "%s: problem too large", what);
    return 0;
}

// The (L, ref_dim) instantiation of a fused kernel: calls f(integral_constant<int, L>, integral_constant<int, ref_dim>).
template <typename F>
inline int dispatch_fused(int L, int ref_dim, F f)
{
    auto levels = [&](auto rd) {
        switch (L) {
            case 1: return f(std::integral_constant<int, 1>(), rd);
            case 2: return f(std::integral_constant<int, 2>(), rd);
            case 3: return f(std::integral_constant<int, 3>(), rd);
            default: return f(std::integral_constant<int, 4>(), rd);
        }
    };
    return ref_dim == 2 ? levels(std::integral_constant<int, 2>()) : levels(std::integral_constant<int, 4>());
}

}  // namespace dfx
