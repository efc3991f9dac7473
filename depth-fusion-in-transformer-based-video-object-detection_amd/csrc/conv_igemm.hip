// Direct convolution as an implicit GEMM on the gfx950 matrix cores (include/dfx_conv.h,
// dfx_conv2d_igemm_f32): the convolutions of the backbones that have no cheaper algorithm here - the 7x7/2
// ResNet stem, the strided 3x3 convolutions, the DFormer depth stem
// (/root/reference/models/backbone_scratch.py:102-141, /root/reference/models/dformer_backbone.py:18-71).
//
//   Y_n[Co, P] = Wp[Co, Kpad] x G_n[Kpad, P],   P = Ho*Wo,   G_n[k, p] = X_n[ci(k), iy(p) + dy(k), ix(p) + dx(k)]
//
// The gathered operand G never exists in memory: a workgroup builds its [BK x BN] slice of it directly in
// LDS.  Thread t owns output pixel n0 + (t & 127) of the tile (so a wave's 64 lanes read 64 neighbouring
// input pixels of one channel / tap: coalesced for stride 1, every other dword for stride 2) and walks 8 of
// the 16 k rows of a K-step; k is wave-uniform, so the tap table entry comes through the scalar cache and
// the bounds test is two unsigned compares per element.  Out-of-map taps read element 0 and are zeroed
// when they are written to LDS, so the loads stay unconditional and in flight across the MFMAs of the
// current K-step.  Everything else is mfma_tile.h: 4 waves x (MT x NT) tiles of v_mfma_f32_32x32x2_f32, BK = 16
// double-buffered, the [m][k] x [k][n] K-step (weights read by ds_read_b128 along k, one read = the operand of
// four MFMAs, the gathered operand by ds_read_b32) and the epilogues (per-row bias + activation into NCHW).
// MFMA-bound: 2*Co*K*P flops per image against 157 TFLOP/s.
#include "dfx_common.h"
#include "dfx_conv.h"
#include "mfma_tile.h"

namespace {

using namespace dfx::mfma;

struct IgemmArgs {
    const float *X = nullptr, *Wp = nullptr;
    const int2 *ktab = nullptr;// per k: {tap index ky*KW+kx (or -1: padding column), byte offset ci*H*W*4 + (ky*dil*W + kx*dil)*4}
    const float *bias = nullptr;
    float *Y = nullptr;
    int Ci = 0, H = 0, W = 0, Co = 0, Ho = 0, Wo = 0, Kpad = 0, stride = 1, pad = 0, act = 0, KH = 1, KW = 1, dil = 1;
    long strideX = 0, strideY = 0;
    int wide = 0;              // Ho*Wo % 4 == 0 and y 16-byte aligned: float4 epilogue through LDS
};

// UT ("uniform tap"): Ci % 16 == 0, so the 16 k of a K-step are 16 input channels of ONE tap: one table entry, one validity
// test and one offset select per K-step instead of eight of each, the eight loads differ in their scalar offset only.  (The
// fp32 MFMA shares the vector lanes - DESIGN.md section 7 - so the ~50 vector instructions and 7 scalar loads this removes
// per K-step were matrix time.)  Everything but the 7x7 stem and the 1-channel DFormer stem takes this path.
template <int BM, int WM, int WN, bool UT>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const IgemmArgs g)
{
    constexpr int BN = 128, BK = 16;
    using T = Tile<BM, BN, WM, WN, 256>;
    constexpr int LDK = BK + 4, LDB = T::LDB;
    constexpr int A_F4 = BM * BK / 4, A_LOADS = (A_F4 + 255) / 256;
    constexpr int B_ROWS = BK / 2;                     // k rows per thread per K-step
    constexpr int A_SZ = BM * LDK, B_SZ = BK * LDB, C_SZ = T::PR * T::LDC;
    constexpr int S_SZ = 2 * (A_SZ + B_SZ) > C_SZ ? 2 * (A_SZ + B_SZ) : C_SZ;
    __shared__ __attribute__((aligned(16))) float smem[S_SZ];        // the two operand stages; the epilogues' transpose buffer
    float (*const As)[A_SZ] = reinterpret_cast<float (*)[A_SZ]>(smem);               // As[buf]: [m][k]
    float (*const Bs)[B_SZ] = reinterpret_cast<float (*)[B_SZ]>(smem + 2 * A_SZ);    // Bs[buf]: [k][n]

    // ---- tile coordinates ---------------------------------------------------------------------------------------------
    const int tid = threadIdx.x;
    const Lane l = lane_of<T>(tid);
    // Tile order (placement only): one-dimensional grid, workgroup ids XCD-remapped (each XCD walks one contiguous range,
    // dfx_common.h), the output-channel block fastest - the Co / BM workgroups that gather the SAME input pixels run back to
    // back on one XCD, so the gathered operand comes from HBM once and from that XCD's L2 afterwards (round 3 measured 3.3x the
    // one-pass traffic with the co block as grid.y: its workgroups landed on whatever XCD the dispatch order gave them).
    const int P = g.Ho * g.Wo, HW = g.H * g.W;
    const int ny = (g.Co + BM - 1) / BM, nx = (P + BN - 1) / BN;
    const int lin = dfx::xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int by = lin % ny, rest = lin / ny;
    const int m0 = by * BM, n0 = (rest % nx) * BN;
    const long bz = __builtin_amdgcn_readfirstlane(rest / nx);      // (scalar: kept in SGPRs, so are the descriptors built from it)

    // ---- operand staging: weights by 16-byte buffer loads, the gathered operand element by element --------------------
    // this thread's output pixel, the top-left input pixel of its receptive field, and a bit per tap that lies
    // inside the map (KH*KW <= 64)
    const int pl = tid & (BN - 1);
    const int kb = __builtin_amdgcn_readfirstlane(tid >> 7);        // 0 / 1: wave-uniform
    const int p = n0 + pl;
    const bool pv = p < P;
    const int oy = (pv ? p : 0) / g.Wo, ox = (pv ? p : 0) - oy * g.Wo;
    const int iy0 = oy * g.stride - g.pad, ix0 = ox * g.stride - g.pad;
    unsigned long long taps = 0;
    if (pv) {
        unsigned rows = 0, cols = 0;
        for (int ky = 0; ky < g.KH; ++ky) rows |= (unsigned)((unsigned)(iy0 + ky * g.dil) < (unsigned)g.H) << ky;
        for (int kx = 0; kx < g.KW; ++kx) cols |= (unsigned)((unsigned)(ix0 + kx * g.dil) < (unsigned)g.W) << kx;
        for (int ky = 0; ky < g.KH; ++ky)
            if ((rows >> ky) & 1u) taps |= (unsigned long long)cols << (ky * g.KW);
    }
    // Buffer loads.  The image descriptor starts `bias_el` elements BEFORE the image, so that the per-lane offset of the
    // receptive field's top-left corner (which lies up to pad rows / columns outside the map) is never negative; the
    // tap's own offset is the scalar offset of the instruction.  A lane whose tap is outside the map gets kOut
    // and the hardware returns 0 for it: no clamp, no select, one shift + compare per element.
    const int bias_el = g.pad * g.W + g.pad;
    const float *Xn = g.X + bz * g.strideX - bias_el;
    const __amdgpu_buffer_rsrc_t rsX = buffer(Xn, ((long)g.Ci * HW + bias_el) * 4);
    const __amdgpu_buffer_rsrc_t rsW = buffer(g.Wp, (long)g.Co * g.Kpad * 4);
    const unsigned vx = (unsigned)(iy0 * g.W + ix0 + bias_el) * 4u;
    unsigned va[A_LOADS];
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
        const int f = tid + i * 256, row = f / (BK / 4), kq = f % (BK / 4), m = m0 + row;
        va[i] = (m < g.Co && f < A_F4) ? ((unsigned)m * (unsigned)g.Kpad + (unsigned)kq * 4u) * 4u : kOut;
    }

    f32x16 acc[T::MT][T::NT] = {};

    f32x4 ra[A_LOADS];
    float rb[B_ROWS];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            ra[i] = load4(rsW, va[i]);
            va[i] += BK * 4u;
        }
        if (UT) {
            const int2 e = g.ktab[k0 + kb];                              // scalar load: k is wave-uniform
            const unsigned vo = ((taps >> (e.x & 63)) & 1ull) ? vx : kOut;
            const int cstep = 2 * HW * 4;                                // k advances by 2 per row of this thread: 2 channels
#pragma unroll
            for (int i = 0; i < B_ROWS; ++i)
                rb[i] = load1(rsX, vo, e.y + i * cstep);
        } else {
#pragma unroll
            for (int i = 0; i < B_ROWS; ++i) {
                const int2 e = g.ktab[k0 + kb + 2 * i];                  // scalar load: k is wave-uniform
                const bool ok = e.x >= 0 && ((taps >> (e.x & 63)) & 1ull);
                rb[i] = load1(rsX, ok ? vx : kOut, e.y);
            }
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int f = tid + i * 256, row = f / (BK / 4), kq = f % (BK / 4);
            if (f >= A_F4) continue;
            *reinterpret_cast<f32x4 *>(&As[buf][row * LDK + kq * 4]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i) Bs[buf][(kb + 2 * i) * LDB + pl] = rb[i];
    };

    // ---- K loop -----------------------------------------------------------------------------------------------------------
    const int steps = g.Kpad / BK;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    for (int t = 0; t < steps; ++t) {
        const int buf = t & 1;
        if (t + 1 < steps) load_tiles((t + 1) * BK);       // in flight during the MFMAs
        kstep_kn<T, BK>(As[buf], Bs[buf], l, acc);
        if (t + 1 < steps) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue dispatch (mfma_tile.h): Y_n[Co][P], per-row bias -------------------------------------------------------
    Epilogue e;
    e.C = g.Y + bz * g.strideY, e.ldc = P;
    e.bias = g.bias, e.bias_per_row = 1;
    e.M = g.Co, e.N = P, e.act = g.act;
    const f32x4 no_prefetch[1] = {};
    if (g.wide && g.act != DFX_ACT_GELU && (long)(g.Co + BM) * P * 4 < (1L << 31)) {
        if (g.bias) return epilogue_lean<T, 2, false, false, false>(smem, acc, l, m0, n0, e, no_prefetch, false);
        return epilogue_lean<T, 0, false, false, false>(smem, acc, l, m0, n0, e, no_prefetch, false);
    }
    if (g.wide) return epilogue_float4<T, false>(smem, acc, l, m0, n0, e, no_prefetch, false);
    epilogue_scalar<T>(acc, l, m0, n0, e);
}

template <int BM, int WM, int WN>
int launch(const IgemmArgs &g, int N, hipStream_t st)
{
    const long blocks = (long)((g.Ho * g.Wo + 127) / 128) * ((g.Co + BM - 1) / BM) * N;
    if (blocks >= (1L << 31)) return dfx::fail(DFX_ERANGE, "conv2d_igemm: too many tiles");
    const dim3 grid((unsigned)blocks), block(256);
    // measurement aid (dfx_profile_*): flops of the launch (K padding included) in the byte field, tag_a = -4
    const long flops = 2L * g.Co * g.Kpad * g.Ho * g.Wo * N;
    if (g.Ci % 16 == 0 && g.Kpad == g.KH * g.KW * g.Ci)
        dfx::launch_timed(flops, -4, BM, conv_igemm_kernel<BM, WM, WN, true>, grid, block, 0, st, g);
    else
        dfx::launch_timed(flops, -4, BM, conv_igemm_kernel<BM, WM, WN, false>, grid, block, 0, st, g);
    return dfx::check_launch("conv_igemm_kernel");
}

}  // namespace

extern "C" int dfx_conv2d_igemm_f32(const float *x, const float *wp, const int *ktab, const float *bias, float *y,
                                    int N, int Ci, int H, int W, int Co, int Ho, int Wo, int Kpad, int KH, int KW,
                                    int stride, int pad, int dilation, int act, long x_image_stride, void *stream)
{
    if (N < 0 || Ci <= 0 || H <= 0 || W <= 0 || Co <= 0 || Ho < 0 || Wo < 0 || Kpad <= 0 || stride <= 0 || pad < 0 ||
        KH <= 0 || KW <= 0 || dilation <= 0)
        return dfx::fail(DFX_EINVAL, "conv2d_igemm: bad dimension");
    if ((long)N * Ho * Wo == 0) return DFX_OK;
    if (!x || !wp || !ktab || !y) return dfx::fail(DFX_EINVAL, "conv2d_igemm: null pointer");
    if (Kpad % 16 || !dfx::aligned16(wp)) return dfx::fail(DFX_EINVAL, "conv2d_igemm: Kpad must be a multiple of 16, wp 16-byte aligned");
    if (KH * KW > 64 || KH > 32 || KW > 32)      // 64-bit tap mask built from 32-bit row and column validity masks
        return dfx::fail(DFX_EINVAL, "conv2d_igemm: at most 64 taps, kernel sides up to 32");
    if (((long)Ci * H * W + (long)pad * W + pad) * 4 >= (1L << 31) || (long)Co * Ho * Wo >= (1L << 31) || (long)Co * Kpad * 4 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "conv2d_igemm: one image's tensor exceeds 2 GiB");
    if (N > 65535) return dfx::fail(DFX_ERANGE, "conv2d_igemm: batch too large");
    if (act < 0 || act > 2) return dfx::fail(DFX_EINVAL, "conv2d_igemm: unknown activation");
    const int wide = ((Ho * Wo) & 3) == 0 && dfx::aligned16(y);
    IgemmArgs g;
    g.X = x, g.Wp = wp, g.ktab = reinterpret_cast<const int2 *>(ktab), g.bias = bias, g.Y = y;
    g.Ci = Ci, g.H = H, g.W = W, g.Co = Co, g.Ho = Ho, g.Wo = Wo, g.Kpad = Kpad;
    g.KH = KH, g.KW = KW, g.stride = stride, g.pad = pad, g.dil = dilation, g.act = act;
    g.strideX = x_image_stride > 0 ? x_image_stride : (long)Ci * H * W, g.strideY = (long)Co * Ho * Wo;
    g.wide = wide;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (Co <= 64) return launch<64, 1, 4>(g, N, st);
    const long t128 = (long)((Co + 127) / 128) * ((Ho * Wo + 127) / 128) * N;
    if (Co % 128 == 0 && t128 >= 2 * 256) return launch<128, 2, 2>(g, N, st);
    return launch<64, 1, 4>(g, N, st);
}
