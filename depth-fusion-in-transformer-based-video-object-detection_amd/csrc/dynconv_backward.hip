// Backward of DynamicConv (csrc/dynconv.hip) in one launch plus a 640-thread reduction (include/dfx_roi.h), gfx950.
//
// Nothing of the forward is saved: per RoI the kernel recomputes Z1 = X K1, A1 = relu(LN(Z1)), Z2 = A1 K2 and then runs
// the four gradient products, all on fp32 MFMA (32 x 32 x 2) with rows padded to 64, in the forward's decomposition: a
// persistent workgroup (4 waves) walks the RoIs, a RoI's matrices live in LDS.
//   P1 Z1  [64,64]  = X   [64,256] K1  [256,64]     2 x 2 tiles, one per wave; Z1 stays in the accumulators until LN1's backward
//   P2 Z2  [64,256] = A1  [64,64]  K2  [64,256]     2 x 8 tiles, four per wave
//   P3 dK2 [64,256] = A1^T[64,64]  dZ2 [64,256]     2 x 8, stored from the accumulators (128-byte row segments)
//   P4 dA1 [64,64]  = dZ2 [64,256] K2^T[256,64]     2 x 2
//   P5 dK1 [256,64] = X^T [256,64] dZ1 [64,64]      8 x 2, four per wave, stored from the accumulators
//   P6 dX  [64,256] = dZ1 [64,64]  K1^T[64,256]     2 x 8, rows < R stored from the accumulators
// LDS over time (38 144 floats = 149 KB of 160):
//   xs [64][260]  X -> Z2 -> dZ2 (in place) -> X again (second staging, an L2 hit) for P5
//   kw 16384      K1 -> K2 -> [64][68] scratch (Zh1) -> K1 again for P6
//   ys [64][68]   Z1 -> A1 -> G1*g1 -> dZ1 (in place)
//   lnp 640, st 128 (LN1's mean and rstd per row)
// K1 / K2 are stored with their 16-byte slots XOR-swizzled by (row & 15): P1 / P2 read them along n (32 consecutive
// floats of one row: the XOR permutes aligned groups of 8 slots, still 32 distinct banks), P4 / P6 read them transposed,
// one ds_read_b128 per lane along the contiguous dimension, lane = row - without the swizzle every lane of a group
// would start on the same bank (row pitches of 256 and 64 floats), with it the 16 lanes of a b128 group (distinct
// lane & 15) hit 16 distinct slots.  A1^T and X^T are read down a column, lanes on neighbouring columns.
// Rows R..63 are padding: X's are zero, dY is loaded as zero there and LN2's pass skips them (their dZ2 rows stay the zero
// rows of xs), which makes dA1, G1 and dZ1 zero rows.
// LayerNorm parameter gradients: per-thread partial sums over the RoIs a workgroup walks, reduced through LDS in a
// fixed order into one row of the [grid, 640] workspace; dynconv_ln_reduce sums the rows in order.  No atomics.
#include "dfx_common.h"
#include "dfx_roi.h"
#include "mfma_tile.h"

namespace {

using namespace dfx::mfma;
constexpr int C = 256, DD = 64, RP = 64;
constexpr int XP = C + 4, YP = DD + 4;
constexpr int X_F4 = (49 * C / 4 + 255) / 256;
constexpr int X_F4_MAX = RP * C / 4 / 256;
constexpr int K_F4 = C * DD / 4 / 256;
constexpr int LN_FLOATS = 2 * DD + 2 * C;

using dfx::sum16;

#define MFMA(A, B, ACC) ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A, B, ACC, 0, 0, 0)
// row of accumulator register r inside a 32 x 32 tile
#define TROW(r) (((r) & 3) + 8 * ((r) >> 2) + 4 * half)

template <int XF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dynamic_conv_backward(
    const float *__restrict__ grad_out, const float *__restrict__ feats, const float *__restrict__ params, long p_stride,
    const float *__restrict__ g1, const float *__restrict__ b1, const float *__restrict__ g2, const float *__restrict__ b2,
    float *__restrict__ grad_feats, float *__restrict__ grad_params, long gp_stride, float *__restrict__ ws, int K, int R,
    float eps)
{
    extern __shared__ float lds[];
    float *xs = lds;                          // [RP][XP]
    float *kw = xs + RP * XP;                 // K1 / K2 (swizzled) / Zh1 scratch [RP][YP]
    float *ys = kw + C * DD;                  // [RP][YP]
    float *lnp = ys + RP * YP;                // g1 b1 g2 b2
    float *st = lnp + LN_FLOATS;              // mean1[64] rstd1[64]
// Thread indices are re-derived from an opaque copy of threadIdx.x at the start of every phase: computed once, the
// compiler hoists the few hundred LDS / global offsets derived from them out of the RoI loop and keeps them in scratch
// memory (239 scratch stores in the prologue, 300 loads per RoI); re-derived, they are a handful of VALU operations.
#define IDS()                                                                                                    \
    int tid_ = threadIdx.x;                                                                                      \
    asm volatile("" : "+v"(tid_));                                                                               \
    const int tid = tid_, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5, mt = wave >> 1,     \
              nh = wave & 1, t16 = tid & 15, rg = tid >> 4;                                                      \
    (void)col; (void)half; (void)mt; (void)nh; (void)t16; (void)rg
    const bool need_f = grad_feats != nullptr, need_p = grad_params != nullptr;

    f32x4 xr[XF], kr[K_F4], dyr[16];
    float dg2a[16], db2a[16], dg1a = 0.f, db1a = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) dg2a[u] = db2a[u] = 0.f;

#define LOAD_X(ROI)                                                                                              \
    do {                                                                                                         \
        const float *xp_ = feats + (long)(ROI) * R * C;                                                          \
        _Pragma("unroll") for (int u = 0; u < XF; ++u) {                                                         \
            const int e = tid + u * 256, row = e >> 6, c4 = e & 63;                                              \
            xr[u] = row < R ? *reinterpret_cast<const f32x4 *>(xp_ + row * C + c4 * 4) : (f32x4){0.f, 0.f, 0.f, 0.f}; \
        }                                                                                                        \
    } while (0)
#define STORE_X()                                                                                                \
    do {                                                                                                         \
        _Pragma("unroll") for (int u = 0; u < XF; ++u) {                                                         \
            const int e = tid + u * 256, row = e >> 6, c4 = e & 63;                                              \
            if (row < R) *reinterpret_cast<f32x4 *>(xs + row * XP + c4 * 4) = xr[u];                             \
        }                                                                                                        \
    } while (0)
#define LOAD_K(PTR)                                                                                              \
    do {                                                                                                         \
        const float *kp_ = (PTR);                                                                                \
        _Pragma("unroll") for (int u = 0; u < K_F4; ++u)                                                         \
            kr[u] = *reinterpret_cast<const f32x4 *>(kp_ + (tid + u * 256) * 4);                                 \
    } while (0)
// SLOTS = 16-byte slots per row: 16 for K1 [256][64], 64 for K2 [64][256]
#define STORE_K(SLOTS)                                                                                           \
    do {                                                                                                         \
        _Pragma("unroll") for (int u = 0; u < K_F4; ++u) {                                                       \
            const int f = tid + u * 256, row = f / (SLOTS), slot = f % (SLOTS);                                  \
            *reinterpret_cast<f32x4 *>(kw + (row * (SLOTS) + (slot ^ (row & 15))) * 4) = kr[u];                  \
        }                                                                                                        \
    } while (0)

    const int tid = threadIdx.x;
    for (int e = tid; e < LN_FLOATS; e += 256)
        lnp[e] = e < DD ? g1[e] : e < 2 * DD ? b1[e - DD] : e < 2 * DD + C ? g2[e - 2 * DD] : b2[e - 2 * DD - C];
    for (int e = tid; e < (RP - R) * (XP / 4); e += 256)      // zero padding rows of X: written once, never overwritten
        *reinterpret_cast<float4 *>(xs + R * XP + e * 4) = make_float4(0.f, 0.f, 0.f, 0.f);

    int roi = blockIdx.x;
    if (roi < K) {
        LOAD_X(roi);
        LOAD_K(params + (long)roi * p_stride);
    }
    for (; roi < K; roi += gridDim.x) {
        const float *prow = params + (long)roi * p_stride;
        const int nxt = roi + (int)gridDim.x;
        {
            IDS();
            STORE_X();
            STORE_K(16);                                                  // K1
        }
        __syncthreads();
        {
            IDS();
            LOAD_K(prow + C * DD);                                        // K2 and dY: in flight during product 1
            const float *gp_ = grad_out + (long)roi * R * C;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int row = rg + 16 * i;
                    dyr[i * 4 + c] = row < R ? *reinterpret_cast<const f32x4 *>(gp_ + row * C + (t16 + 16 * c) * 4)
                                             : (f32x4){0.f, 0.f, 0.f, 0.f};
                }
        }
        // ---- P1: Z1 = X K1 ----
        f32x16 z1;
#pragma unroll
        for (int r = 0; r < 16; ++r) z1[r] = 0.f;
        {
            IDS();
            const float *arow = xs + (mt * 32 + col) * XP + half * 4;
            const int n = nh * 32 + col, ns = n >> 2, nl = n & 3;
#pragma unroll 2
            for (int j = 0; j < C / 8; ++j) {
                const float4 a = *reinterpret_cast<const float4 *>(arow + j * 8);
                float bq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = j * 8 + half * 4 + q;
                    bq[q] = kw[k * DD + ((ns ^ (k & 15)) << 2) + nl];
                }
                MFMA(a.x, bq[0], z1);
                MFMA(a.y, bq[1], z1);
                MFMA(a.z, bq[2], z1);
                MFMA(a.w, bq[3], z1);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) ys[(mt * 32 + TROW(r)) * YP + nh * 32 + col] = z1[r];
        }
        __syncthreads();
        // ---- LN1 + ReLU on the rows of Z1 -> A1; mean and rstd kept for the backward ----
        {
        IDS();
        for (int row = rg; row < RP; row += 16) {
            const float4 gg = *reinterpret_cast<const float4 *>(lnp + t16 * 4);
            const float4 bb = *reinterpret_cast<const float4 *>(lnp + DD + t16 * 4);
            float4 v = *reinterpret_cast<const float4 *>(ys + row * YP + t16 * 4);
            const float mean = sum16(v.x + v.y + v.z + v.w) * (1.f / DD);
            v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
            const float rstd = rsqrtf(sum16(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w) * (1.f / DD) + eps);
            *reinterpret_cast<float4 *>(ys + row * YP + t16 * 4) =
                make_float4(fmaxf(v.x * rstd * gg.x + bb.x, 0.f), fmaxf(v.y * rstd * gg.y + bb.y, 0.f),
                            fmaxf(v.z * rstd * gg.z + bb.z, 0.f), fmaxf(v.w * rstd * gg.w + bb.w, 0.f));
            if (t16 == 0) {
                st[row] = mean;
                st[RP + row] = rstd;
            }
        }
        STORE_K(64);                                                      // K2 (K1's last read was before the barrier above)
        }
        __syncthreads();
        // ---- P2: Z2 = A1 K2 -> xs (X was last read in P1) ----
        {
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            IDS();
            const float *arow = ys + (mt * 32 + col) * YP + half * 4;
#pragma unroll 1
            for (int j = 0; j < DD / 8; ++j) {
                const float4 a = *reinterpret_cast<const float4 *>(arow + j * 8);
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = j * 8 + half * 4 + q;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int n = nh * 128 + t * 32 + col;
                        MFMA(av[q], kw[k * C + (((n >> 2) ^ (k & 15)) << 2) + (n & 3)], acc[t]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mt * 32 + TROW(r);
                    if (row < R) xs[row * XP + nh * 128 + t * 32 + col] = acc[t][r];
                }
        }
        __syncthreads();
        // ---- LN2 forward and backward on the rows of Z2: xs <- dZ2 (rows < R; the padding stays zero) ----
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            IDS();
            const int row = rg + 16 * i;
            // padding rows have G2 = 0: nothing to add, nothing to store.  The branch is uniform per 16-lane row group, which is
            // all that sum16 exchanges between
            if (row < R) {
                float4 v[4];
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    v[c] = *reinterpret_cast<const float4 *>(xs + row * XP + (t16 + 16 * c) * 4);
                    s += v[c].x + v[c].y + v[c].z + v[c].w;
                }
                const float mean = sum16(s) * (1.f / C);
                float sq = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    v[c].x -= mean; v[c].y -= mean; v[c].z -= mean; v[c].w -= mean;
                    sq += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
                }
                const float rstd = rsqrtf(sum16(sq) * (1.f / C) + eps);
                float zh[16], h[16], s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 gg = *reinterpret_cast<const float4 *>(lnp + 2 * DD + (t16 + 16 * c) * 4);
                    const float4 bb = *reinterpret_cast<const float4 *>(lnp + 2 * DD + C + (t16 + 16 * c) * 4);
                    const float vv[4] = {v[c].x, v[c].y, v[c].z, v[c].w}, gv[4] = {gg.x, gg.y, gg.z, gg.w},
                                bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int u = c * 4 + e;
                        zh[u] = vv[e] * rstd;
                        const float G = zh[u] * gv[e] + bv[e] > 0.f ? dyr[i * 4 + c][e] : 0.f;
                        h[u] = G * gv[e];
                        s1 += h[u];
                        s2 += h[u] * zh[u];
                        dg2a[u] += G * zh[u];
                        db2a[u] += G;
                    }
                }
                const float m1 = sum16(s1) * (1.f / C), m2 = sum16(s2) * (1.f / C);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    *reinterpret_cast<float4 *>(xs + row * XP + (t16 + 16 * c) * 4) =
                        make_float4(rstd * (h[c * 4] - m1 - zh[c * 4] * m2), rstd * (h[c * 4 + 1] - m1 - zh[c * 4 + 1] * m2),
                                    rstd * (h[c * 4 + 2] - m1 - zh[c * 4 + 2] * m2), rstd * (h[c * 4 + 3] - m1 - zh[c * 4 + 3] * m2));
            }
            __builtin_amdgcn_sched_barrier(0);      // one row at a time: interleaved rows put their temporaries into scratch
        }
        __syncthreads();
        // second staging of this RoI's X (for P5) and K1 (for P6), in flight during P3 / P4 - or, when neither runs, the next
        // RoI's operands (issued here and not earlier: the staging registers and dY's are then never live together)
        {
            IDS();
            if (need_p || need_f) {
                if (need_p) LOAD_X(roi);
                if (need_f) LOAD_K(prow);
            } else if (nxt < K) {
                LOAD_X(nxt);
                LOAD_K(params + (long)nxt * p_stride);
            }
        }
        // ---- P3: dK2 = A1^T dZ2, stored from the accumulators ----
        if (need_p) {
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            IDS();
            const float *acol = ys + half * 4 * YP + mt * 32 + col;
            const float *bcol = xs + half * 4 * XP + nh * 128 + col;
#pragma unroll 1
            for (int j = 0; j < RP / 8; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float a = acol[(j * 8 + q) * YP];
#pragma unroll
                    for (int t = 0; t < 4; ++t) MFMA(a, bcol[(j * 8 + q) * XP + t * 32], acc[t]);
                }
            float *gp_ = grad_params + (long)roi * gp_stride + C * DD;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) gp_[(mt * 32 + TROW(r)) * C + nh * 128 + t * 32 + col] = acc[t][r];
        }
        // ---- P4: dA1 = dZ2 K2^T ----
        f32x16 da;
#pragma unroll
        for (int r = 0; r < 16; ++r) da[r] = 0.f;
        {
            IDS();
            const float *arow = xs + (mt * 32 + col) * XP + half * 4;
            const int n = nh * 32 + col;
            const float *brow = kw + n * C;
#pragma unroll 2
            for (int j = 0; j < C / 8; ++j) {
                const float4 a = *reinterpret_cast<const float4 *>(arow + j * 8);
                const float4 b = *reinterpret_cast<const float4 *>(brow + (((2 * j + half) ^ (n & 15)) << 2));
                MFMA(a.x, b.x, da);
                MFMA(a.y, b.y, da);
                MFMA(a.z, b.z, da);
                MFMA(a.w, b.w, da);
            }
        }
        __syncthreads();                      // ys (A1) and kw (K2) were read by P3 / P4 of every wave
        // ---- LN1 backward, elementwise part in the accumulator layout: ys <- G1*g1, kw scratch <- Zh1 ----
        {
            IDS();
            const int cidx = nh * 32 + col;
            const float g = lnp[cidx];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mt * 32 + TROW(r);
                const float zh = (z1[r] - st[row]) * st[RP + row];
                const float G = ys[row * YP + cidx] > 0.f ? da[r] : 0.f;
                dg1a += G * zh;
                db1a += G;
                ys[row * YP + cidx] = G * g;
                kw[row * YP + cidx] = zh;
            }
        }
        if (need_p || need_f) {
            __syncthreads();
            IDS();
            for (int row = rg; row < RP; row += 16) {
                const float4 h = *reinterpret_cast<const float4 *>(ys + row * YP + t16 * 4);
                const float4 z = *reinterpret_cast<const float4 *>(kw + row * YP + t16 * 4);
                const float m1 = sum16(h.x + h.y + h.z + h.w) * (1.f / DD);
                const float m2 = sum16(h.x * z.x + h.y * z.y + h.z * z.z + h.w * z.w) * (1.f / DD);
                const float rstd = st[RP + row];
                *reinterpret_cast<float4 *>(ys + row * YP + t16 * 4) =
                    make_float4(rstd * (h.x - m1 - z.x * m2), rstd * (h.y - m1 - z.y * m2), rstd * (h.z - m1 - z.z * m2),
                                rstd * (h.w - m1 - z.w * m2));
            }
            __syncthreads();
            if (need_p) STORE_X();            // rows < R over dZ2; the padding rows are still zero
            if (need_f) STORE_K(16);
            __syncthreads();
            if (nxt < K) {                    // the next RoI's X and K1: in flight during P5 / P6
                LOAD_X(nxt);
                LOAD_K(params + (long)nxt * p_stride);
            }
            // ---- P5: dK1 = X^T dZ1, stored from the accumulators ----
            if (need_p) {
                f32x16 acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
                IDS();
                const float *acol = xs + half * 4 * XP + mt * 128 + col;
                const float *bcol = ys + half * 4 * YP + nh * 32 + col;
#pragma unroll 1
                for (int j = 0; j < RP / 8; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float b = bcol[(j * 8 + q) * YP];
#pragma unroll
                        for (int t = 0; t < 4; ++t) MFMA(acol[(j * 8 + q) * XP + t * 32], b, acc[t]);
                    }
                float *gp_ = grad_params + (long)roi * gp_stride;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) gp_[(mt * 128 + t * 32 + TROW(r)) * DD + nh * 32 + col] = acc[t][r];
            }
            // ---- P6: dX = dZ1 K1^T, rows < R stored from the accumulators ----
            if (need_f) {
                f32x16 acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
                IDS();
                const float *arow = ys + (mt * 32 + col) * YP + half * 4;
#pragma unroll 1
                for (int j = 0; j < DD / 8; ++j) {
                    const float4 a = *reinterpret_cast<const float4 *>(arow + j * 8);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int n = nh * 128 + t * 32 + col;
                        const float4 b = *reinterpret_cast<const float4 *>(kw + n * DD + (((2 * j + half) ^ (n & 15)) << 2));
                        MFMA(a.x, b.x, acc[t]);
                        MFMA(a.y, b.y, acc[t]);
                        MFMA(a.z, b.z, acc[t]);
                        MFMA(a.w, b.w, acc[t]);
                    }
                }
                float *gx_ = grad_feats + (long)roi * R * C;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = mt * 32 + TROW(r);
                        if (row < R) gx_[row * C + nh * 128 + t * 32 + col] = acc[t][r];
                    }
            }
        }
        __syncthreads();                      // xs / kw / ys are rewritten at the top of the loop
    }
    // ---- this workgroup's LayerNorm parameter gradients: fixed-order reduction through LDS -> ws[blockIdx][640] ----
    {
        IDS();
        float *red2 = xs;                     // [16 row groups][dg2 256 | db2 256]
        float *red1 = xs + 16 * 2 * C;        // [4 (mt, half)][dg1 64 | db1 64]
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red2[rg * 2 * C + (t16 + 16 * c) * 4 + e] = dg2a[c * 4 + e];
                red2[rg * 2 * C + C + (t16 + 16 * c) * 4 + e] = db2a[c * 4 + e];
            }
        red1[(mt * 2 + half) * 2 * DD + nh * 32 + col] = dg1a;
        red1[(mt * 2 + half) * 2 * DD + DD + nh * 32 + col] = db1a;
        __syncthreads();
        for (int e = tid; e < LN_FLOATS; e += 256) {
            float s = 0.f;
            if (e < 2 * DD) {
                for (int p = 0; p < 4; ++p) s += red1[p * 2 * DD + e];
            } else {
                for (int p = 0; p < 16; ++p) s += red2[p * 2 * C + e - 2 * DD];
            }
            ws[(long)blockIdx.x * LN_FLOATS + e] = s;
        }
    }
}

#undef LOAD_X
#undef STORE_X
#undef LOAD_K
#undef STORE_K
#undef MFMA
#undef TROW
#undef IDS

__global__ __launch_bounds__(LN_FLOATS) void dynconv_ln_reduce(const float *__restrict__ ws, float *__restrict__ grad_ln,
                                                               int rows)
{
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += ws[r * LN_FLOATS + threadIdx.x];
    grad_ln[threadIdx.x] = s;
}

}  // namespace

extern "C" int dfx_dynamic_conv_backward_f32(const float *grad_out, const float *feats, const float *params, long p_stride,
                                             const float *g1, const float *b1, const float *g2, const float *b2,
                                             float *grad_feats, float *grad_params, long gp_stride, float *grad_ln,
                                             float *workspace, int K, int R, int Cc, int dd, float eps, void *stream)
{
    if (K < 0 || R <= 0) return dfx::fail(DFX_EINVAL, "dynamic_conv_backward: bad dimension");
    if (Cc != C || dd != DD || R > RP)
        return dfx::fail(DFX_EINVAL, "dynamic_conv_backward: built for C = 256, dim_dynamic = 64, at most 64 rows per RoI "
                                     "(got C=%d dd=%d R=%d)", Cc, dd, R);
    if (!grad_ln || !workspace) return dfx::fail(DFX_EINVAL, "dynamic_conv_backward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K == 0) {
        if (hipMemsetAsync(grad_ln, 0, sizeof(float) * LN_FLOATS, st) != hipSuccess)
            return dfx::fail(DFX_ELAUNCH, "dynamic_conv_backward: cannot zero grad_ln");
        return DFX_OK;
    }
    if (!grad_out || !feats || !params || !g1 || !b1 || !g2 || !b2)
        return dfx::fail(DFX_EINVAL, "dynamic_conv_backward: null pointer");
    if (p_stride < 2L * C * DD || (p_stride & 3) || !dfx::aligned16(grad_out) || !dfx::aligned16(feats) ||
        !dfx::aligned16(params) || !dfx::aligned16(g1) || !dfx::aligned16(b1) || !dfx::aligned16(g2) || !dfx::aligned16(b2) ||
        !dfx::aligned16(grad_feats) || !dfx::aligned16(grad_params) || !dfx::aligned16(grad_ln) || !dfx::aligned16(workspace) ||
        (grad_params && (gp_stride < 2L * C * DD || (gp_stride & 3))))
        return dfx::fail(DFX_EINVAL, "dynamic_conv_backward: params / grad_params rows must hold 2*C*dd floats, 16-byte aligned buffers");
    const size_t lds = sizeof(float) * (RP * XP + C * DD + RP * YP + LN_FLOATS + 2 * RP);
    if (const int rc = dfx::raise_lds_limit<&dynamic_conv_backward<X_F4>, &dynamic_conv_backward<X_F4_MAX>>(
            "dynamic_conv_backward", 160 * 1024))
        return rc;
    const int grid = K < 256 ? K : 256;         // one persistent workgroup per CU; fixed for a given K: reproducible sums
    if (R <= 49)
        hipLaunchKernelGGL(dynamic_conv_backward<X_F4>, dim3(grid), dim3(256), lds, st, grad_out, feats, params, p_stride, g1,
                           b1, g2, b2, grad_feats, grad_params, gp_stride, workspace, K, R, eps);
    else
        hipLaunchKernelGGL(dynamic_conv_backward<X_F4_MAX>, dim3(grid), dim3(256), lds, st, grad_out, feats, params, p_stride,
                           g1, b1, g2, b2, grad_feats, grad_params, gp_stride, workspace, K, R, eps);
    hipLaunchKernelGGL(dynconv_ln_reduce, dim3(1), dim3(LN_FLOATS), 0, st, workspace, grad_ln, grid);
    return dfx::check_launch("dynamic_conv_backward");
}
