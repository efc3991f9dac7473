// Fused MSDA front end + sampling, backward (training), for gfx950.
//
// The backward of dfx_msda_fused_forward_f32 (msda_fused.hip) from the forward's own raw inputs: the two
// Linear outputs (offsets, logits), the reference points and the value map.  Nothing else is saved by the
// caller: the kernel recomputes the softmax weights with the forward's arithmetic and the sampling locations by
// calling the forward's routines (msda_tap.h: load_ref, sample_location), so sampling_locations /
// attention_weights never exist in HBM in either direction.
//
// Mapping: msda_bwd_m8d32's (msda_backward.hip) - one wave per query, lane = (head, channel quad), the 32
// channels of a head in 8 adjacent lanes x 4 registers, reductions over them by 3 xor shuffles (head_sum).
// The gradient of one sample (corner<> and the block around it) is kept in this file, next to msda_bwd_m8d32's:
// moved into a routine both kernels call, hipcc packs and contracts its products differently and grad_off,
// grad_logits, grad_ref and grad_loc change in the last bit.
// The 4*LT softmax weights of the lane's head and the 4*LT gradients g_a with respect to them stay in
// registers (LT levels and P = 4 points are compile-time), which is all the softmax backward needs:
//     grad_logits[k] = a[k] * (g_a[k] - sum_j a[j] * g_a[j]).
// With s = the head-summed derivative of the output with respect to a PIXEL coordinate, the gradient of a
// location is g_x = W_l * s_x, g_y = H_l * s_y (as in msda_bwd_m8d32) and
//     ref_dim 2: grad_off = (g_x / W_l, g_y / H_l) = (s_x, s_y)   - no multiply-then-divide round trip
//     ref_dim 4: grad_off = (g_x * ref_w, g_y * ref_h) * 0.5 / 4
//     grad_ref[q,l,0:2] = sum over heads and points of (g_x, g_y)
//     grad_ref[q,l,2:4] = sum over heads and points of (g_x * off_x, g_y * off_y) * 0.5 / 4   (ref_dim 4)
// the sum over the 8 heads being three more xor shuffles across the wave.
//
// No atomics on the small gradients: every element of grad_off, grad_logits and grad_ref belongs to exactly
// one wave, which writes it with a plain store - all of them, also for samples outside the map (zeros) - so
// the caller allocates the three buffers uninitialised and two calls give the same bits.  Only grad_value is
// shared between queries and is accumulated with hardware float atomics into a zero-filled buffer; when the
// caller passes none (the memory is detached) the NEED_VALUE = false instantiation contains no atomic and no
// corner store at all.
//
// Deterministic mode (fixed_sum.h): the accumulation of grad_value is a compile-time policy.  FloatSum is the route above;
// FixedSum adds to_fixed(the same fp32 product) by return-less 64-bit integer atomics into a caller-owned, zero-filled
// int64 [N,S,M,D] workspace - same lane map, the 8 lanes of a head add 256 contiguous bytes - which one streaming kernel
// (fixed_sum.hip) converts to fp32 grad_value.  The three small gradients do not touch the policy and keep their bits.
#include "dfx_common.h"
#include "fixed_sum.h"
#include "msda_tap.h"

namespace {

using dfx::all_heads_sum;
using dfx::head_sum;
using dfx::xcd_remap;

// Filled by name in the entry point, passed by value.
struct FusedBwdArgs {
    const float *value;
    const int64_t *shapes, *lsi;
    const float *ref, *off, *logits, *grad_out;
    float *grad_value, *grad_off, *grad_logits, *grad_ref;      // grad_value, grad_ref: may be null
    long off_stride, logit_stride, goff_stride, glog_stride;
    int NQ, Lq, S;
    // FixedSum only (after the float route's fields, whose kernel-argument offsets stay): workspace, scale word, F
    unsigned long long *fixed_ws;
    const void *scratch;
    int F;
};

// How a lane adds one fp32 product into grad_value: the element type of the buffer it adds into, that buffer, the add.
// `up` is 2^(F-e) of fixed_sum.h and means nothing to the float route.
struct FloatSum {
    using type = float;
    __device__ __forceinline__ static float *base(const FusedBwdArgs &g) { return g.grad_value; }
    __device__ __forceinline__ static double scale(const FusedBwdArgs &) { return 0.; }
    __device__ __forceinline__ static void add(float *p, float x, double) { unsafeAtomicAdd(p, x); }
};
struct FixedSum {
    using type = unsigned long long;            // the int64 workspace, laid out like grad_value
    __device__ __forceinline__ static type *base(const FusedBwdArgs &g) { return g.fixed_ws; }
    __device__ __forceinline__ static double scale(const FusedBwdArgs &g) { return dfx::fixed::load_scale(g.scratch, g.F).up; }
    __device__ __forceinline__ static void add(type *p, float x, double up) { atomicAdd(p, dfx::fixed::to_fixed(x, up)); }
};

// One bilinear corner: its share of d out / d (h, w, weight) and, with NEED_VALUE, of grad_value.
template <bool NEED_VALUE, typename SUM>
__device__ __forceinline__ void corner(const float *__restrict__ vl, typename SUM::type *__restrict__ gl, double up, int o,
                                       float wgt, float GH, float GW, const float4 &t, float4 &gh, float4 &gw, float4 &val)
{
    const float4 v = *reinterpret_cast<const float4 *>(vl + o);
    gh.x += GH * v.x; gh.y += GH * v.y; gh.z += GH * v.z; gh.w += GH * v.w;
    gw.x += GW * v.x; gw.y += GW * v.y; gw.z += GW * v.z; gw.w += GW * v.w;
    val.x += wgt * v.x; val.y += wgt * v.y; val.z += wgt * v.z; val.w += wgt * v.w;
    if constexpr (NEED_VALUE) {
        SUM::add(gl + o, wgt * t.x, up);
        SUM::add(gl + o + 1, wgt * t.y, up);
        SUM::add(gl + o + 2, wgt * t.z, up);
        SUM::add(gl + o + 3, wgt * t.w, up);
    }
}

template <int LT, int REFDIM, bool NEED_VALUE, typename SUM = FloatSum>
__global__ __launch_bounds__(256) void msda_fused_bwd(const FusedBwdArgs g)
{
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int qi = blk * 4 + (threadIdx.x >> 6);
    if (qi >= g.NQ) return;                     // whole wave leaves together: shuffles below are safe
    const int m = lane >> 3, cg = lane & 7;
    const int b = qi / g.Lq;
    const long chan = (long)b * g.S * 256 + m * 32 + cg * 4;
    const float4 top = *reinterpret_cast<const float4 *>(g.grad_out + (long)qi * 256 + lane * 4);

    const double up = SUM::scale(g);

    // every level's size up front, as the taps kernels do: read per level between the stores and atomics of the loop
    // below they cost two VGPRs (the struct's pointers carry no __restrict__) and, at L = 2, a wave per SIMD
    dfx::LevelDims<LT> lv;
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        lv.H[l] = (int)g.shapes[2 * l];
        lv.W[l] = (int)g.shapes[2 * l + 1];
        lv.R[l] = (int)g.lsi[l];
    }

    // ---- softmax over the head's L*P logits: the forward's arithmetic restated (msda_fused.hip says why), keep the two alike
    float a[LT * 4], ga[LT * 4];
    {
        const float *lg = g.logits + (long)qi * g.logit_stride + m * (LT * 4);
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < LT; ++k) {
            const float4 e = *reinterpret_cast<const float4 *>(lg + k * 4);
            a[k * 4] = e.x; a[k * 4 + 1] = e.y; a[k * 4 + 2] = e.z; a[k * 4 + 3] = e.w;
            mx = fmaxf(mx, fmaxf(fmaxf(e.x, e.y), fmaxf(e.z, e.w)));
        }
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < LT * 4; ++k) {
            a[k] = expf(a[k] - mx);
            sum += a[k];
        }
#pragma unroll
        for (int k = 0; k < LT * 4; ++k) a[k] = a[k] / sum;
    }

#pragma unroll
    for (int l = 0; l < LT; ++l) {
        const int H = lv.H[l], W = lv.W[l];
        const long lvl = chan + (long)lv.R[l] * 256;
        const float *vl = g.value + lvl;
        typename SUM::type *gl = NEED_VALUE ? SUM::base(g) + lvl : nullptr;
        const dfx::RefPoint r = dfx::load_ref<REFDIM>(g.ref + ((long)qi * LT + l) * REFDIM);
        const float4 *op = reinterpret_cast<const float4 *>(g.off + (long)qi * g.off_stride + (m * LT + l) * 8);
        const float4 o01 = op[0], o23 = op[1];
        const float ox[4] = {o01.x, o01.z, o23.x, o23.z}, oy[4] = {o01.y, o01.w, o23.y, o23.w};
        float gox[4], goy[4];
        float rgx = 0.f, rgy = 0.f, rgw = 0.f, rgh = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float2 xy = dfx::sample_location<REFDIM>(r, ox[p], oy[p], W, H);
            const float h_im = xy.y * (float)H - 0.5f;
            const float w_im = xy.x * (float)W - 0.5f;
            const float weight = a[l * 4 + p];
            float s_w = 0.f, s_h = 0.f, g_a = 0.f;
            // the in-range test depends on (query, head) only: uniform over the 8 lanes of a head
            if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
                const float hf = floorf(h_im), wf = floorf(w_im);
                const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
                const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
                const float4 t = make_float4(top.x * weight, top.y * weight, top.z * weight, top.w * weight);
                float4 gh = make_float4(0.f, 0.f, 0.f, 0.f), gw = gh, val = gh;
                if (h0 >= 0 && w0 >= 0) corner<NEED_VALUE, SUM>(vl, gl, up, (h0 * W + w0) * 256, hh * hw, -hw, -hh, t, gh, gw, val);
                if (h0 >= 0 && w1 <= W - 1) corner<NEED_VALUE, SUM>(vl, gl, up, (h0 * W + w1) * 256, hh * lw, -lw, hh, t, gh, gw, val);
                if (h1 <= H - 1 && w0 >= 0) corner<NEED_VALUE, SUM>(vl, gl, up, (h1 * W + w0) * 256, lh * hw, hw, -lh, t, gh, gw, val);
                if (h1 <= H - 1 && w1 <= W - 1) corner<NEED_VALUE, SUM>(vl, gl, up, (h1 * W + w1) * 256, lh * lw, lw, lh, t, gh, gw, val);
                g_a = top.x * val.x + top.y * val.y + top.z * val.z + top.w * val.w;
                s_w = gw.x * t.x + gw.y * t.y + gw.z * t.z + gw.w * t.w;
                s_h = gh.x * t.x + gh.y * t.y + gh.z * t.z + gh.w * t.w;
            }
            s_w = head_sum(s_w);
            s_h = head_sum(s_h);
            ga[l * 4 + p] = head_sum(g_a);
            const float g_x = (float)W * s_w, g_y = (float)H * s_h;      // gradient of the location
            if (REFDIM == 2) {
                gox[p] = s_w;
                goy[p] = s_h;
            } else {
                gox[p] = g_x * r.kx * 0.5f / 4.f;
                goy[p] = g_y * r.ky * 0.5f / 4.f;
                rgw += g_x * ox[p];
                rgh += g_y * oy[p];
            }
            rgx += g_x;
            rgy += g_y;
        }
        if (cg == l) {      // the 8 lanes of a head hold the same sums: lane l of the head stores level l
            float4 *gp = reinterpret_cast<float4 *>(g.grad_off + (long)qi * g.goff_stride + (m * LT + l) * 8);
            gp[0] = make_float4(gox[0], goy[0], gox[1], goy[1]);
            gp[1] = make_float4(gox[2], goy[2], gox[3], goy[3]);
        }
        if (g.grad_ref) {   // wave-uniform
            rgx = all_heads_sum(rgx);
            rgy = all_heads_sum(rgy);
            float *gr = g.grad_ref + ((long)qi * LT + l) * REFDIM;
            if (REFDIM == 2) {
                if (lane == l) *reinterpret_cast<float2 *>(gr) = make_float2(rgx, rgy);
            } else {
                rgw = all_heads_sum(rgw);
                rgh = all_heads_sum(rgh);
                if (lane == l) *reinterpret_cast<float4 *>(gr) = make_float4(rgx, rgy, rgw * 0.5f / 4.f, rgh * 0.5f / 4.f);
            }
        }
    }

    // ---- softmax backward on the registers
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < LT * 4; ++k) dot += a[k] * ga[k];
    float *gq = g.grad_logits + (long)qi * g.glog_stride + m * (LT * 4);
#pragma unroll
    for (int k = 0; k < LT; ++k)
        if (cg == k)
            *reinterpret_cast<float4 *>(gq + k * 4) =
                make_float4(a[k * 4] * (ga[k * 4] - dot), a[k * 4 + 1] * (ga[k * 4 + 1] - dot),
                            a[k * 4 + 2] * (ga[k * 4 + 2] - dot), a[k * 4 + 3] * (ga[k * 4 + 3] - dot));
}

template <int LT, int REFDIM, bool NEED_VALUE, typename SUM = FloatSum>
int launch(const FusedBwdArgs &g, hipStream_t st)
{
    hipLaunchKernelGGL((msda_fused_bwd<LT, REFDIM, NEED_VALUE, SUM>), dim3((unsigned)((g.NQ + 3) / 4)), dim3(256), 0, st, g);
    return dfx::check_launch("msda_fused_bwd");
}

// Both entry points.  fixed_ws == nullptr: the float route (grad_value accumulated into, may be null).  Otherwise the
// fixed-point route: grad_value is WRITTEN from the workspace's sums.
int backward(const char *what, const float *value, const int64_t *shapes, const int64_t *lsi, const float *ref, int ref_dim,
             const float *off, long off_stride, const float *logits, long logit_stride, const float *grad_out, int N, int S,
             int M, int D, int L, int Lq, int P, float *grad_value, long long *fixed_ws, void *scratch, float *grad_off,
             long grad_off_stride, float *grad_logits, long grad_logit_stride, float *grad_ref, hipStream_t st)
{
    const int rc = dfx::check_fused(what, "dfx_msda_backward_f32", value, shapes, lsi, ref, ref_dim, off, off_stride, logits,
                                    logit_stride, grad_out, N, S, M, D, L, Lq, P);
    if (rc < 0) return rc;
    const long nvalue = (long)N * S * M * D;
    if (rc == 1) {      // no query: nothing is added; the fixed route owes its caller the zeros it would have converted
        if (fixed_ws && nvalue > 0 && hipMemsetAsync(grad_value, 0, sizeof(float) * nvalue, st) != hipSuccess)
            return dfx::fail(DFX_ELAUNCH, "%s: memset failed", what);
        return DFX_OK;
    }
    if (!grad_off || !grad_logits) return dfx::fail(DFX_EINVAL, "%s: null gradient buffer", what);
    const long orow = (long)M * L * P * 2, lrow = (long)M * L * P;
    if (grad_off_stride < orow || grad_logit_stride < lrow || ((grad_off_stride | grad_logit_stride) & 3))
        return dfx::fail(DFX_EINVAL, "%s: bad row strides", what);
    if (!dfx::aligned16(grad_value) || !dfx::aligned16(grad_off) || !dfx::aligned16(grad_logits) || !dfx::aligned16(grad_ref))
        return dfx::fail(DFX_EINVAL, "%s: buffers must be 16-byte aligned", what);
    const long nq = (long)N * Lq;
    if (S == 0) {
        if (hipMemset2DAsync(grad_off, sizeof(float) * grad_off_stride, 0, sizeof(float) * orow, nq, st) != hipSuccess ||
            hipMemset2DAsync(grad_logits, sizeof(float) * grad_logit_stride, 0, sizeof(float) * lrow, nq, st) != hipSuccess ||
            (grad_ref && hipMemsetAsync(grad_ref, 0, sizeof(float) * nq * L * ref_dim, st) != hipSuccess))
            return dfx::fail(DFX_ELAUNCH, "%s: memset failed", what);
        return DFX_OK;
    }
    FusedBwdArgs g{};
    g.value = value; g.shapes = shapes; g.lsi = lsi; g.ref = ref; g.off = off; g.logits = logits; g.grad_out = grad_out;
    g.grad_value = grad_value; g.grad_off = grad_off; g.grad_logits = grad_logits; g.grad_ref = grad_ref;
    g.off_stride = off_stride; g.logit_stride = logit_stride; g.goff_stride = grad_off_stride; g.glog_stride = grad_logit_stride;
    g.NQ = (int)nq; g.Lq = Lq; g.S = S;
    if (!fixed_ws)
        return dfx::dispatch_fused(L, ref_dim, [&](auto lt, auto rd) {
            constexpr int LT = decltype(lt)::value, RD = decltype(rd)::value;
            return grad_value ? launch<LT, RD, true>(g, st) : launch<LT, RD, false>(g, st);
        });
    g.fixed_ws = reinterpret_cast<unsigned long long *>(fixed_ws);
    g.scratch = scratch;
    g.F = dfx::fixed::fraction_bits(dfx::fixed::msda_terms(Lq));
    if (const int e = dfx::fixed::enqueue_absmax(what, grad_out, nq * M * D, scratch, st)) return e;
    const int e = dfx::dispatch_fused(L, ref_dim, [&](auto lt, auto rd) {
        return launch<decltype(lt)::value, decltype(rd)::value, true, FixedSum>(g, st);
    });
    return e ? e : dfx::fixed::enqueue_convert(what, fixed_ws, scratch, g.F, grad_value, nvalue, st);
}

}  // namespace

extern "C" int dfx_msda_fused_backward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                                           const float *ref, int ref_dim, const float *off, long off_stride,
                                           const float *logits, long logit_stride, const float *grad_out, int N,
                                           int S, int M, int D, int L, int Lq, int P, float *grad_value,
                                           float *grad_off, long grad_off_stride, float *grad_logits,
                                           long grad_logit_stride, float *grad_ref, void *stream)
{
    return backward("msda fused backward", value, shapes, lsi, ref, ref_dim, off, off_stride, logits, logit_stride, grad_out, N,
                    S, M, D, L, Lq, P, grad_value, nullptr, nullptr, grad_off, grad_off_stride, grad_logits, grad_logit_stride,
                    grad_ref, static_cast<hipStream_t>(stream));
}

extern "C" int dfx_msda_fused_backward_fixed_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                                                 const float *ref, int ref_dim, const float *off, long off_stride,
                                                 const float *logits, long logit_stride, const float *grad_out, int N,
                                                 int S, int M, int D, int L, int Lq, int P, float *grad_value,
                                                 long long *workspace, void *scratch, float *grad_off,
                                                 long grad_off_stride, float *grad_logits, long grad_logit_stride,
                                                 float *grad_ref, void *stream)
{
    const char *what = "msda fused backward (fixed)";
    if (!grad_value || !workspace || !scratch)
        return dfx::fail(DFX_EINVAL, "%s: null grad_value, workspace or scratch word (without a value gradient call "
                                     "dfx_msda_fused_backward_f32 with grad_value == NULL)", what);
    if (!dfx::aligned16(workspace) || !dfx::aligned16(scratch)) return dfx::fail(DFX_EINVAL, "%s: buffers must be 16-byte aligned", what);
    return backward(what, value, shapes, lsi, ref, ref_dim, off, off_stride, logits, logit_stride, grad_out, N, S, M, D, L, Lq, P,
                    grad_value, workspace, scratch, grad_off, grad_off_stride, grad_logits, grad_logit_stride, grad_ref,
                    static_cast<hipStream_t>(stream));
}
