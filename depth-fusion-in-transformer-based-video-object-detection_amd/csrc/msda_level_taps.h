// Per-query arithmetic and LDS image geometry of the level-in-LDS MSDA kernels (gfx950): the forward
// (msda_level.hip) and the grad_value kernel of its backward (msda_level_backward.hip) include this, so
// both see one softmax, one location rule and one token index per sample.
//
// LDS image (both kernels): a bordered (H+3) x (W+2) token map, two planes of 16-byte chunks, plane c
// holding channels 4c..4c+3 of the workgroup's channel octet, plane stride plane_tokens(H, W).  A tap's
// token index tb = y0 * (W+2) + x0 is relative to image token (1, 1); y0 is in [-1, H] and x0 in [-1, W]
// whatever the inputs are (make_taps clamps the pixel coordinate in float first), so the four corners
// tb, tb+1, tb+W+2, tb+W+3 lie in image tokens 0 .. (H+3)*(W+2), all inside the plane.
#pragma once
#include "dfx_common.h"

namespace dfx {
namespace level {

constexpr int THREADS = 1024;
constexpr long LDS_CAP = 160 * 1024;

typedef float v2f __attribute__((ext_vector_type(2)));      // v_pk_{mul,add,fma}_f32 operands

__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f splat(float x) { return (v2f){x, x}; }

struct Taps {
    int tb[4];          // y0 * (W+2) + x0 of each point (>= -(W+3)): token index relative to image token (1, 1)
    v2f wt[4], wb[4];   // corner weights {(y0,x0), (y0,x1)} and {(y1,x0), (y1,x1)}, attention weight folded in
};

// The Linear outputs of one (query, head) as loaded: 4 logits, 4 (x, y) offsets, the reference point.
struct Raw {
    float4 lg, o01, o23, r;
};

template <int REFDIM>
__device__ __forceinline__ Raw load_raw(const float *__restrict__ rp, const float *__restrict__ op,
                                        const float *__restrict__ lp)
{
    Raw w;
    w.lg = *reinterpret_cast<const float4 *>(lp);
    w.o01 = *reinterpret_cast<const float4 *>(op);
    w.o23 = *reinterpret_cast<const float4 *>(op + 4);
    if (REFDIM == 2) {
        const float2 r = *reinterpret_cast<const float2 *>(rp);
        w.r = make_float4(r.x, r.y, 0.f, 0.f);
    } else {
        w.r = *reinterpret_cast<const float4 *>(rp);
    }
    return w;
}

// exp(x) for x <= 0 (logit - max), two at a time: 2^t * (1 + f ln2) with t = RN(x log2e) and f the
// rounding error of that product (an fma away) - v_exp_f32's 1 ulp plus ~1e-8 |x|, without libm's
// range reduction (x is clamped at -87, where the result is 1e-38).
__device__ __forceinline__ v2f exp_neg(v2f x)
{
    x.x = fmaxf(x.x, -87.f);
    x.y = fmaxf(x.y, -87.f);
    const v2f L2E = splat(1.4426950216293335f);
    const v2f t = x * L2E;
    const v2f f = pk_fma(x, L2E, -t) * splat(0.6931471805599453f);
    const v2f e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    return pk_fma(e, f, e);
}

// Per-thread constants of the level.
struct Level {
    v2f size, rsize;    // (W, H) and their correctly rounded reciprocals
    int H, W, WB;
};

__device__ __forceinline__ Level make_level(int H, int W)
{
    Level lv;
    lv.size = (v2f){(float)W, (float)H};
    lv.rsize = (v2f){1.f / (float)W, 1.f / (float)H};
    lv.H = H; lv.W = W; lv.WB = W + 2;
    return lv;
}

// One (query, head): softmax over the 4 logits (F.softmax, ms_deform_attn.py:99), locations
// ref + off / (W, H) or ref_xy + off / P * ref_wh * 0.5 (:102-110), pixel coordinates and bilinear
// weights (ms_deform_im2col_cuda.cuh:33-84, :281-291).  Written on (x, y) pairs so that it compiles
// to packed fp32 instructions; the two divisions per point are q = o*r, q += (o - q*size)*r with
// r = RN(1/size), which is the correctly rounded quotient (Markstein), and the softmax quotient is
// the same iteration on a Newton-refined v_rcp_f32.
template <int REFDIM>
__device__ __forceinline__ Taps make_taps(const Raw &in, const Level &lv)
{
    const float mx = fmaxf(fmaxf(in.lg.x, in.lg.y), fmaxf(in.lg.z, in.lg.w));
    const v2f e01 = exp_neg((v2f){in.lg.x - mx, in.lg.y - mx});
    const v2f e23 = exp_neg((v2f){in.lg.z - mx, in.lg.w - mx});
    float sum = 0.f;
    sum += e01.x; sum += e01.y; sum += e23.x; sum += e23.y;
    float y0 = __builtin_amdgcn_rcpf(sum);
    y0 = fmaf(fmaf(-sum, y0, 1.f), y0, y0);
    const v2f ys = splat(y0), ss = splat(sum);
    v2f a01 = e01 * ys, a23 = e23 * ys;
    a01 = pk_fma(pk_fma(-a01, ss, e01), ys, a01);
    a23 = pk_fma(pk_fma(-a23, ss, e23), ys, a23);
    const float aw[4] = {a01.x, a01.y, a23.x, a23.y};
    const v2f o[4] = {{in.o01.x, in.o01.y}, {in.o01.z, in.o01.w}, {in.o23.x, in.o23.y}, {in.o23.z, in.o23.w}};
    const v2f rxy = {in.r.x, in.r.y}, rwh = {in.r.z, in.r.w};
    Taps t;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        v2f loc;
        if (REFDIM == 2) {
            v2f q = o[p] * lv.rsize;
            q = pk_fma(pk_fma(-q, lv.size, o[p]), lv.rsize, q);
            loc = rxy + q;
        } else {
            loc = rxy + o[p] * splat(0.25f) * rwh * splat(0.5f);
        }
        const v2f im = pk_fma(loc, lv.size, splat(-0.5f));               // (w_im, h_im)
        // clamp to [-1, size]: NaN and -inf land on -1 (zero border, weight 0), +inf on `size` (dropped below)
        const float ws = __builtin_amdgcn_fmed3f(im.x, -1.f, lv.size.x);
        const float hs = __builtin_amdgcn_fmed3f(im.y, -1.f, lv.size.y);
        int ix, iy;                                                      // floor to int in one instruction
        asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ix) : "v"(ws));
        asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(iy) : "v"(hs));
        const v2f l = {__builtin_amdgcn_fractf(ws), __builtin_amdgcn_fractf(hs)};   // (lw, lh) = x - floor(x), exact
        const v2f hc = splat(1.f) - l;                                   // (hw, hh)
        // the skip rule -1 < h_im < H, -1 < w_im < W: a sample at exactly -1 has weight 0 on its only
        // in-map row/column already, so only the upper bounds are left to test
        const float aa = (iy < lv.H && ix < lv.W) ? aw[p] : 0.f;
        const v2f xw = {hc.x, l.x};                                      // (hw, lw)
        t.wt[p] = splat(hc.y) * xw * splat(aa);
        t.wb[p] = splat(l.y) * xw * splat(aa);
        // iy * WB + ix; the (+1, +1) of the border is folded into the image base by the caller (rows 0..H+1)
        asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(t.tb[p]) : "v"(iy), "v"(lv.WB), "v"(ix));
    }
    return t;
}

// plane stride in tokens: bordered tokens rounded up to 4 mod 8
inline long plane_tokens(int H, int W)
{
    const long nt = (long)(H + 3) * (W + 2);        // one token of border, one more row for y1 of dropped samples
    return nt + 1 + ((4 - (nt + 1) % 8) + 8) % 8;
}

// CUs of the device current at the call rounded down to a multiple of 8: the persistent grids of both kernels
// (item & 7, the head, is then fixed per workgroup and the 4 octets of one (frame, head) stay on one XCD / L2).
// Both callers keep the first call's answer in a function-local static, so a process that drives GPUs of
// different sizes runs every one of them with the first one's grid: correct for any grid (the item loop
// covers the rest), tuned only for that device.
inline int persistent_grid()
{
    return cu_count() / 8 * 8;
}

}  // namespace level
}  // namespace dfx
