// Multi-scale deformable attention, forward, for gfx950 (MI355X / CDNA4).
//
// Replaces /root/reference/models/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299 (kernel)
// and ms_deform_attn_cuda.cu:20-80 (host) behind the C ABI in include/dfx_msda.h.
//
// The reference gives one THREAD one output channel (1024-thread blocks, int64 shape loads and
// scalar 4-byte gathers per thread, every thread redoing the sample geometry).  Here the unit of
// work is a WAVE and the work is split in two phases (production geometry M=8 heads x D=32
// channels, P=4 points; msda_fwd_taps<LT, V, WIDE> for a value map of dtype V = fp32, bf16 or fp16,
// locations and weights always fp32; the figures below are the fp32 ones):
//
//   phase A  "taps": lane = one (query, level, point, head) sample of the wave's 2 queries.  It
//            loads its (x, y, weight) triple - the 64 lanes read 768 contiguous bytes - and does
//            the geometry ONCE: skip rule, floor, corner validity, 4 byte offsets, 4 weights
//            premultiplied by the attention weight.  Taps go to LDS in [query][level][point][head]
//            order (32 bytes each; two 16-byte stores).
//   phase B  "gather": lane = (head m = lane>>3, channel quad cg = lane&7).  Per point it reads
//            its head's tap back as two 16-byte LDS broadcasts (8 distinct addresses, 128
//            contiguous bytes: conflict-free), then issues the 4 corner fetches as 16-byte loads
//            with a wave-uniform base + 32-bit offset; the 8 lanes of a head read one contiguous
//            128-byte value row, so a wave-instruction touches 8 rows.  16 gathers per level are
//            in flight before the first FMA; the reduction over L*P samples stays in registers
//            and the query's 1 KiB output row leaves as one float4 per lane.  (msda_tap.h,
//            gather_query; a 2-byte V halves every size here: 512-byte token rows, 8-byte loads,
//            64-byte head rows, and it has a second, 16-byte gather - see below.)
//
// A 256-thread workgroup holds 4 waves x 2 queries = 8 consecutive queries (x `iters`);
// workgroups are remapped so that each XCD walks a contiguous raster range of queries and its
// private L2 holds only that band of the value map (dfx_common.h).  The earlier one-phase form
// (every lane redoing the geometry) measured VALU-bound at ~1000 instructions per query; it is
// kept (msda_fwd_m8d32) only for what the taps kernel does not take: P != 4, L > 4, a loc that is
// not 8-byte aligned.
//
// Roofline: HBM-bound gather.  Algorithmic bytes per call
//   4 * (N*S*M*D  +  3*N*Lq*M*L*P  +  N*Lq*M*D)       (value + loc/aw + out, fp32)
// = 10.21 MB per frame for the encoder geometry (S = Lq = 4200, L = 1).
//
// 2-byte value maps (bf16 / fp16, dfx_msda_{forward,backward}_{bf16,f16}): the mixed-precision form of
// the operator - what MSDeformAttn hands the op under torch.autocast - value from a Linear (bf16 /
// fp16), sampling locations and attention weights in fp32 (include/dfx_msda.h, dfx_msda_forward_bf16).
// Only the value map, grad_output and the forward output are 2-byte; the arithmetic is the fp32 op's:
// corner weights, products and the sum over L*P samples in fp32, one rounding per output element
// (a plain conversion, v_cvt_pk_{bf16,f16}_f32).  Backward accumulates grad_value into an fp32
// buffer with float atomics (a packed 2-byte atomic would round at every add).
//
//   forward, M = 8, D = 32, P = 4, L <= 4, 16-byte aligned value / out: msda_fwd_taps<LT, bf16 / fp16>, the
//            kernel above (launch errors name it msda_half_fwd_taps, as they always have).  Phase A is the
//            same code with 512-byte token rows; phase B gathers each corner as 2-byte channels, accumulates
//            in fp32 registers and stores the output row in the value dtype.  Two gather widths, the same bits:
//              wide    4 lanes x 16 B per head: 8 channels a lane, both queries of the wave in one pass
//              narrow  8 lanes x  8 B per head: 4 channels a lane, one query per pass (the fp32 mapping)
//            wide for L = 1 (bf16, 32 frames: enc 98 us against 130, dec 12.9 against 14.2), narrow for more
//            levels (enc L4: 601 us against 621; wide holds 16 corner rows of 16 B per level in flight and
//            needs 178-256 VGPRs at L >= 2, so it is built for L = 1 only).  DFX_MSDA_HALF_NARROW=1 takes
//            narrow for every L (A/B).
//   forward, anything else: msda_fwd_generic<bf16 / fp16>, one thread per output element, scalar 2-byte
//            reads (odd D, any alignment).
//   backward (msda_backward.hip), M = 8, D = 32, 16-byte aligned value / grad_out: msda_bwd_m8d32<bf16 /
//            fp16> (8-byte corner and grad_out reads); anything else msda_bwd_generic<bf16 / fp16>.
//
// Algorithmic bytes of a 2-byte forward call: 2*N*S*M*D + 12*N*Lq*M*L*P + 2*N*Lq*M*D
// (5.91 MB per encoder frame, S = Lq = 4200, L = 1; 10.21 MB in fp32).
#include "dfx_common.h"
#include "msda_tap.h"

namespace {

using dfx::Acc;
using dfx::fma4;
using dfx::narrow4;
using dfx::Pack;
using dfx::Tap;
using dfx::xcd_remap;

// ---------------------------------------------------------------------------------------------
// Fast path: M = 8, D = 32, fp32, 16-byte aligned buffers, any P and L (run-time values; scalar
// loc / aw loads).  One phase: a wave = one query, lane = (head, channel quad), every lane does the
// geometry of its head's samples itself.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void msda_fwd_m8d32(const float *__restrict__ value,
                                                      const int64_t *__restrict__ shapes,
                                                      const int64_t *__restrict__ lsi,
                                                      const float *__restrict__ loc,
                                                      const float *__restrict__ aw,
                                                      int NQ, int Lq, int S, int L, int P,
                                                      float *__restrict__ out)
{
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int qi = blk * 4 + (threadIdx.x >> 6);   // flat query index over N*Lq
    if (qi >= NQ) return;
    const int m = lane >> 3, cg = lane & 7;
    const long samp = (long)qi * 8 + m;            // flat (b,q,m) index
    // the batch element's slab, plus this lane's channel quad inside a head's 128 bytes
    const char *vb = reinterpret_cast<const char *>(value) + (size_t)(qi / Lq) * S * 1024 + cg * 16;
    const float *lp = loc + samp * (long)(L * P * 2);
    const float *ap = aw + samp * (long)(L * P);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], R = (int)lsi[l];
        for (int p = 0; p < P; ++p) {
            const float lx = lp[(l * P + p) * 2], ly = lp[(l * P + p) * 2 + 1];
            const Tap t = dfx::make_tap<1024u>(lx, ly, ap[l * P + p], H, W, R, m * 128);
            const float4 v0 = *reinterpret_cast<const float4 *>(vb + t.off.x);
            const float4 v1 = *reinterpret_cast<const float4 *>(vb + t.off.y);
            const float4 v2 = *reinterpret_cast<const float4 *>(vb + t.off.z);
            const float4 v3 = *reinterpret_cast<const float4 *>(vb + t.off.w);
            fma4(acc, t.w.x, v0); fma4(acc, t.w.y, v1); fma4(acc, t.w.z, v2); fma4(acc, t.w.w, v3);
        }
    }
    *reinterpret_cast<float4 *>(out + (long)qi * 256 + m * 32 + cg * 4) = acc;
}

// ---------------------------------------------------------------------------------------------
// Fast path: M = 8, D = 32, P = 4, LT levels (1..4) known at compile time; value / out of dtype V
// (fp32, bf16, fp16), fp32 loc / aw.  Token rows are 256 * sizeof(V) bytes.  A 256-thread
// workgroup = 4 waves x 2 queries.  WIDE (2-byte V, LT = 1 only) is the 16-byte gather.
// ---------------------------------------------------------------------------------------------
template <int LT, typename V, bool WIDE>
__global__ __launch_bounds__(256) void msda_fwd_taps(const V *__restrict__ value,
                                                     const int64_t *__restrict__ shapes,
                                                     const int64_t *__restrict__ lsi,
                                                     const float *__restrict__ loc,
                                                     const float *__restrict__ aw, int NQ, int Lq,
                                                     int S, int iters, V *__restrict__ out)
{
    static_assert(!WIDE || (LT == 1 && sizeof(V) == 2), "the wide gather serves 2-byte values at L = 1 only");
    constexpr int QW = 2;                 // queries per wave per iteration
    constexpr int TAPS = QW * LT * 32;    // taps per wave per iteration (multiple of 64)
    constexpr unsigned ROW = 256u * sizeof(V);   // bytes of one token row (8 heads x 32 channels)
    __shared__ uint4 s_off[4][TAPS];
    __shared__ float4 s_w[4][TAPS];
    // wave index as a scalar: everything derived from it (query index, batch element, the value
    // slab pointer) then lives in SGPRs and the gathers use scalar-base + 32-bit-offset addressing
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    uint4 *toff = s_off[wave];
    float4 *tw = s_w[wave];
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned slab = (unsigned)S * ROW;      // bytes of one batch element's value map

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
        dfx::write_taps<LT, QW, ROW>(loc, aw, q0, NQ, lane, lv, toff, tw);
        dfx::wave_lds_fence();
        // ---- phase B: gather ----
        if (WIDE) {
            // lane = (query qq = lane>>5, head m = (lane>>2)&7, channel octet cg = lane&3); the pair may
            // straddle two batch elements, so the second one's slab goes into the lane's offset
            // (< 2 * slab <= S * 1024 < 2^32: the launcher's bound).  A query past NQ has zero taps.
            const int b0 = q0 / Lq;
            const char *vb = reinterpret_cast<const char *>(value) + (size_t)b0 * slab;
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
                Pack<V, 8> v[16];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    v[p * 4 + 0] = *reinterpret_cast<const Pack<V, 8> *>(vb + (o[p].x + lane_b));
                    v[p * 4 + 1] = *reinterpret_cast<const Pack<V, 8> *>(vb + (o[p].y + lane_b));
                    v[p * 4 + 2] = *reinterpret_cast<const Pack<V, 8> *>(vb + (o[p].z + lane_b));
                    v[p * 4 + 3] = *reinterpret_cast<const Pack<V, 8> *>(vb + (o[p].w + lane_b));
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float wk[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const Pack<V, 8> &c = v[p * 4 + k];
                        fma4(lo, wk[k], make_float4((float)c.v[0], (float)c.v[1], (float)c.v[2], (float)c.v[3]));
                        fma4(hi, wk[k], make_float4((float)c.v[4], (float)c.v[5], (float)c.v[6], (float)c.v[7]));
                    }
                }
            }
            if (qi < NQ) {
                const Pack<V, 4> a = narrow4<V>(lo), c = narrow4<V>(hi);
                Pack<V, 8> r;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    r.v[k] = a.v[k];
                    r.v[4 + k] = c.v[k];
                }
                *reinterpret_cast<Pack<V, 8> *>(out + (long)qi * 256 + (lane & 31) * 8) = r;
            }
        } else {
            // lane = (head m = lane>>3, channel quad cg = lane&7), one query per pass
            const int m = lane >> 3;
            const unsigned lane_b = (unsigned)(lane & 7) * (unsigned)(4 * sizeof(V));
#pragma unroll
            for (int qq = 0; qq < QW; ++qq) {
                const int qi = q0 + qq;
                if (qi < NQ) {
                    const char *vq = reinterpret_cast<const char *>(value) + (size_t)(qi / Lq) * slab;
                    const float4 acc = dfx::gather_query<LT, V>(vq, lane_b, m, toff + qq * LT * 32, tw + qq * LT * 32);
                    *reinterpret_cast<Pack<V, 4> *>(out + (long)qi * 256 + lane * 4) = narrow4<V>(acc);
                }
            }
        }
        dfx::wave_lds_fence();   // the next iteration overwrites the taps
    }
}

// ---------------------------------------------------------------------------------------------
// Generic path: any M, D, L, P; every value dtype (arithmetic in Acc<V>, one rounding at the store).
// One thread per output element, channel fastest (adjacent lanes read adjacent channels of the same
// value row), grid-stride.  Used by the reference's tiny test fixture (M=D=2), odd head sizes,
// unaligned buffers and every fp64 call.
// ---------------------------------------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(256) void msda_fwd_generic(const V *__restrict__ value,
                                                        const int64_t *__restrict__ shapes,
                                                        const int64_t *__restrict__ lsi,
                                                        const Acc<V> *__restrict__ loc,
                                                        const Acc<V> *__restrict__ aw, long total, int S,
                                                        int M, int D, int L, int Lq, int P,
                                                        V *__restrict__ out)
{
    using T = Acc<V>;
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
        const V *vb = value + (long)b * S * row + m * D + c;
        long wp = samp * L * P, lp = wp * 2;
        T col = 0;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const V *vl = vb + (long)((int)lsi[l]) * row;
            for (int p = 0; p < P; ++p, ++wp, lp += 2) {
                const T h_im = loc[lp + 1] * (T)H - (T)0.5;
                const T w_im = loc[lp] * (T)W - (T)0.5;
                if (h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W) {
                    const T hf = floor(h_im), wf = floor(w_im);
                    const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
                    const T lh = h_im - hf, lw = w_im - wf, hh = (T)1 - lh, hw = (T)1 - lw;
                    T v1 = 0, v2 = 0, v3 = 0, v4 = 0;
                    if (h0 >= 0 && w0 >= 0) v1 = (T)vl[(long)(h0 * W + w0) * row];
                    if (h0 >= 0 && w1 <= W - 1) v2 = (T)vl[(long)(h0 * W + w1) * row];
                    if (h1 <= H - 1 && w0 >= 0) v3 = (T)vl[(long)(h1 * W + w0) * row];
                    if (h1 <= H - 1 && w1 <= W - 1) v4 = (T)vl[(long)(h1 * W + w1) * row];
                    col += (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4) * aw[wp];
                }
            }
        }
        out[idx] = static_cast<V>(col);
    }
}

// One host path for every value dtype: argument checks, the empty problem and the generic fallback
// are shared, and so is the taps fast path of fp32, bf16 and fp16 (fp32 alone has msda_fwd_m8d32 behind it,
// fp64 has no fast path).  Launch-error texts name the kernel as they always have.
template <typename V>
int forward_impl(const V *value, const int64_t *shapes, const int64_t *lsi, const Acc<V> *loc, const Acc<V> *aw,
                 int N, int S, int M, int D, int L, int Lq, int P, V *out, void *stream)
{
    constexpr bool half = sizeof(V) == 2;
    // an empty value map (S = 0) may come to the 2-byte entry points as a null pointer: nothing of it is read
    const int rc = dfx::check_dims(half && S == 0 ? static_cast<const void *>(out) : value, shapes, lsi, loc, aw, out,
                                   N, S, M, D, L, Lq, P);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long nq = (long)N * Lq;
    if (S == 0 || L == 0 || P == 0) {   // nothing to sample: the reference returns zeros
        if (hipMemsetAsync(out, 0, sizeof(V) * nq * M * D, st) != hipSuccess)
            return dfx::fail(DFX_ELAUNCH, half ? "msda forward (2-byte value): memset failed"
                                               : "msda forward: memset failed");
        return DFX_OK;
    }
    if constexpr (!std::is_same<V, double>::value) {   // fp64 always takes the generic kernel
        // S * 1024 < 2^32 keeps a tap offset plus a second batch element's slab (2-byte wide gather) in 32 bits
        const bool fast = M == 8 && D == 32 && nq < (1L << 28) && (long)S * 1024 < (1L << 32) &&
                          dfx::aligned16(value) && dfx::aligned16(out);
        if (fast && P == 4 && L <= 4 && (reinterpret_cast<uintptr_t>(loc) & 7u) == 0) {
            const dfx::TapsGrid tg = dfx::taps_grid(nq);
            const bool wide = half && L == 1 && !dfx::tuning().msda_half_narrow;
#define DFX_TAPS(LT, WIDE)                                                                                  \
            hipLaunchKernelGGL((msda_fwd_taps<LT, V, WIDE>), dim3(tg.blocks), dim3(256), 0, st, value, shapes, lsi, \
                               loc, aw, (int)nq, Lq, S, tg.iters, out)
            if constexpr (half) {   // the wide gather is built for 2-byte values at L = 1 only
                if (wide) DFX_TAPS(1, true);
            }
            if (!wide) {
                switch (L) {
                    case 1: DFX_TAPS(1, false); break;
                    case 2: DFX_TAPS(2, false); break;
                    case 3: DFX_TAPS(3, false); break;
                    default: DFX_TAPS(4, false); break;
                }
            }
#undef DFX_TAPS
            return dfx::check_launch(half ? "msda_half_fwd_taps" : "msda_fwd_taps");
        }
        if constexpr (!half) {
            if (fast) {
                const int grid = (int)((nq + 3) / 4);
                hipLaunchKernelGGL(msda_fwd_m8d32, dim3(grid), dim3(256), 0, st, value, shapes, lsi,
                                   loc, aw, (int)nq, Lq, S, L, P, out);
                return dfx::check_launch("msda_fwd_m8d32");
            }
        }
    }
    const long total = nq * M * D;
    hipLaunchKernelGGL((msda_fwd_generic<V>), dim3(dfx::grid_for(total)), dim3(256), 0, st, value, shapes, lsi, loc,
                       aw, total, S, M, D, L, Lq, P, out);
    return dfx::check_launch(half ? "msda_half_fwd_generic"
                                  : sizeof(V) == 4 ? "msda_fwd_generic<float>" : "msda_fwd_generic<double>");
}

}  // namespace

extern "C" int dfx_msda_forward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                                    const float *loc, const float *aw, int N, int S, int M, int D,
                                    int L, int Lq, int P, float *out, void *stream)
{
    return forward_impl<float>(value, shapes, lsi, loc, aw, N, S, M, D, L, Lq, P, out, stream);
}

extern "C" int dfx_msda_forward_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                                    const double *loc, const double *aw, int N, int S, int M, int D,
                                    int L, int Lq, int P, double *out, void *stream)
{
    return forward_impl<double>(value, shapes, lsi, loc, aw, N, S, M, D, L, Lq, P, out, stream);
}

extern "C" int dfx_msda_forward_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                     const float *loc, const float *aw, int N, int S, int M, int D, int L, int Lq,
                                     int P, uint16_t *out, void *stream)
{
    return forward_impl<__hip_bfloat16>(reinterpret_cast<const __hip_bfloat16 *>(value), shapes, lsi, loc, aw, N, S,
                                        M, D, L, Lq, P, reinterpret_cast<__hip_bfloat16 *>(out), stream);
}

extern "C" int dfx_msda_forward_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                    const float *loc, const float *aw, int N, int S, int M, int D, int L, int Lq,
                                    int P, uint16_t *out, void *stream)
{
    return forward_impl<_Float16>(reinterpret_cast<const _Float16 *>(value), shapes, lsi, loc, aw, N, S, M, D, L,
                                  Lq, P, reinterpret_cast<_Float16 *>(out), stream);
}

extern "C" int dfx_abi_version(void) { return 5; }

extern "C" int dfx_profile_enable(int on)
{
    dfx::profile_state().enabled = on != 0;
    return DFX_OK;
}

extern "C" int dfx_profile_drain(float *ms, long *bytes, int *tag_a, int *tag_b, int cap)
{
    dfx::ProfileState &p = dfx::profile_state();
    std::lock_guard<std::mutex> lock(p.mu);
    int n = 0;
    for (auto &r : p.records) {
        float t = -1.f;
        if (hipEventSynchronize(r.stop) == hipSuccess) (void)hipEventElapsedTime(&t, r.start, r.stop);
        if (n < cap) {
            if (ms) ms[n] = t;
            if (bytes) bytes[n] = r.bytes;
            if (tag_a) tag_a[n] = r.tag_a;
            if (tag_b) tag_b[n] = r.tag_b;
            ++n;
        }
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    p.records.clear();
    return n;
}

extern "C" const char *dfx_last_error(void) { return dfx::err_slot(); }

extern "C" int dfx_tuning_reload(void)
{
    dfx::tuning_slot().read();
    return DFX_OK;
}
