// bf16 GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulation) for the opt-in bf16 FFNs of
// the inference path (include/dfx_gemm_bf16.h):  C = act(A x W^T + bias (+ R)),  A fp32 or bf16, W bf16 [N,K], C fp32 or bf16.
//
// Structure (CDNA4, wave64), the fp32 GEMM's with another operand type (mfma_tile.h: tile geometry, accumulator layout, K-step
// and epilogues):
//   workgroup = 256 threads = 2 x 2 waves over a 128 x 128 (or 64 x 64) output tile;
//   K is walked in steps of BK = 32 through a double-buffered LDS stage As[buf][m][k], Bs[buf][n][k] of bf16 (row pitch 40
//   elements = five 16-byte slots).  A thread stages chunks of 8 consecutive k: 16 bytes of a bf16 operand as they are, 32 bytes of
//   an fp32 A rounded to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) on their way to LDS - no bf16 copy of the activations ever
//   reaches memory.  The next step's global loads are issued before the MFMAs of the current one and written to the other buffer
//   after them: one barrier per K-step.
//   Operands are read through buffer descriptors of their exact extents with 32-bit byte offsets; what lies outside the problem
//   (rows beyond M or N, chunks beyond K) gets an offset beyond every extent and arrives as zeros.
//   Epilogue: + bias, + residual, activation in fp32; one rounding when C is bf16.  No atomics, no split-K: a result element is one
//   MFMA chain in ascending k, so two calls give the same bits.
// These products are meant to be HBM-bound (256 -> 1024: ~170 flop/byte against a bf16 ridge of ~310): workgroup ids are
// XCD-remapped with n fastest, so the tiles that share an A panel run on one XCD and the panel is fetched from memory once.
#include "dfx_common.h"
#include "dfx_gemm_bf16.h"
#include "mfma_tile.h"

namespace {

using namespace dfx::mfma;

struct Args {
    const void *A = nullptr;
    long lda = 0;
    const unsigned short *W = nullptr;
    long ldw = 0;
    const float *bias = nullptr;
    const float *R = nullptr;
    long ldr = 0;
    void *C = nullptr;
    long ldc = 0;
    int c_bf16 = 0;
    int M = 0, N = 0, K = 0, act = 0;
    int wide = 0;             // N % 8 == 0, rows of C (and R) 16-byte aligned: the 8-column epilogue
    int nx = 0;               // tiles along N
};

constexpr int BK = 32, LDK = BK + 8, CH = BK / 8;       // K-step, LDS row pitch (elements), 8-element chunks per row and step

template <int BM, int BN, bool A_BF16>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const Args g)
{
    using T = Tile<BM, BN, 2, 2, 256>;
    constexpr int NTHR = 256, MT = T::MT, NT = T::NT;
    constexpr int A_SZ = BM * LDK, B_SZ = BN * LDK;                     // bf16 elements per stage
    constexpr int A_L = BM * CH / NTHR, B_L = BN * CH / NTHR;           // chunks per thread
    static_assert(BM * CH % NTHR == 0 && BN * CH % NTHR == 0, "whole chunks per thread");
    constexpr int STAGE_BYTES = 2 * (A_SZ + B_SZ) * 2, C_BYTES = T::PR * T::LDC * 4;
    constexpr int S_BYTES = STAGE_BYTES > C_BYTES ? STAGE_BYTES : C_BYTES;
    // one LDS object: the two operand stages, re-used by the epilogue as a [64][BN + 4] fp32 transpose buffer
    __shared__ __attribute__((aligned(16))) float smem[S_BYTES / 4];
    unsigned short *const stage = reinterpret_cast<unsigned short *>(smem);
    auto As = [&](int buf) { return stage + buf * A_SZ; };
    auto Bs = [&](int buf) { return stage + 2 * A_SZ + buf * B_SZ; };

    const int tid = threadIdx.x;
    const Lane l = lane_of<T>(tid);
    const int lin = dfx::xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int m0 = (lin / g.nx) * BM, n0 = (lin % g.nx) * BN;
    constexpr unsigned ES = A_BF16 ? 2u : 4u;                             // bytes per element of A

    const rsrc_t rsA = buffer(g.A, ((long)(g.M - 1) * g.lda + g.K) * ES);
    const rsrc_t rsW = buffer(g.W, ((long)(g.N - 1) * g.ldw + g.K) * 2);
    // chunk f = tid + i * 256 of a stage is row f / CH, k = 8 (f % CH) .. + 7: the thread's k offset is the same for all its chunks
    const int kq = (tid % CH) * 8;
    unsigned va[A_L], vb[B_L];
#pragma unroll
    for (int i = 0; i < A_L; ++i) {
        const int m = m0 + (tid + i * NTHR) / CH;
        va[i] = m < g.M ? ((unsigned)m * (unsigned)g.lda + (unsigned)kq) * ES : kOut;
    }
#pragma unroll
    for (int i = 0; i < B_L; ++i) {
        const int n = n0 + (tid + i * NTHR) / CH;
        vb[i] = n < g.N ? ((unsigned)n * (unsigned)g.ldw + (unsigned)kq) * 2u : kOut;
    }

    f32x4 ra[A_L][A_BF16 ? 1 : 2], rb[B_L];
    auto load_tiles = [&](int k0) {
        const bool in_k = k0 + kq < g.K;                                 // (K % 8 == 0: a chunk lies inside or outside)
#pragma unroll
        for (int i = 0; i < A_L; ++i) {
            const unsigned o = in_k ? va[i] + (unsigned)k0 * ES : kOut;
            ra[i][0] = load4(rsA, o);
            if (!A_BF16) ra[i][A_BF16 ? 0 : 1] = load4(rsA, in_k ? o + 16u : kOut);
        }
#pragma unroll
        for (int i = 0; i < B_L; ++i) rb[i] = load4(rsW, in_k ? vb[i] + (unsigned)k0 * 2u : kOut);
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_L; ++i) {
            const int row = (tid + i * NTHR) / CH;
            const u32x4 v = A_BF16 ? __builtin_bit_cast(u32x4, ra[i][0]) : pack_bf16x8(ra[i][0], ra[i][A_BF16 ? 0 : 1]);
            *reinterpret_cast<u32x4 *>(As(buf) + row * LDK + kq) = v;
        }
#pragma unroll
        for (int i = 0; i < B_L; ++i) {
            const int row = (tid + i * NTHR) / CH;
            *reinterpret_cast<u32x4 *>(Bs(buf) + row * LDK + kq) = __builtin_bit_cast(u32x4, rb[i]);
        }
    };

    f32x16 acc[MT][NT] = {};
    const int steps = (g.K + BK - 1) / BK;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    for (int t = 0; t < steps; ++t) {
        const int buf = t & 1;
        if (t + 1 < steps) load_tiles((t + 1) * BK);          // in flight during the MFMAs below
        kstep_bf16<T, BK>(As(buf), Bs(buf), l, acc);
        if (t + 1 < steps) store_tiles(buf ^ 1);
        __syncthreads();
    }

    EpilogueOut e;
    e.C = g.C, e.ldc = g.ldc;
    e.R = g.R, e.ldr = g.ldr;
    e.bias = g.bias;
    e.M = g.M, e.N = g.N, e.act = g.act;
    if (g.wide) {
        if (g.c_bf16) epilogue_oct<T, true>(smem, acc, l, m0, n0, e);
        else epilogue_oct<T, false>(smem, acc, l, m0, n0, e);
    } else {
        if (g.c_bf16) epilogue_scalar_out<T, true>(acc, l, m0, n0, e);
        else epilogue_scalar_out<T, false>(acc, l, m0, n0, e);
    }
}

template <int BM, int BN>
int launch(Args g, int a_bf16, hipStream_t st)
{
    g.nx = (g.N + BN - 1) / BN;
    const long total = (long)g.nx * ((g.M + BM - 1) / BM);
    if (total >= (1L << 31)) return dfx::fail(DFX_ERANGE, "gemm_bf16: too many tiles");
    const dim3 grid((unsigned)total), block(256);
    // measurement aid (dfx_profile_*): flops of the launch in the byte field, tag_a = -5, tag_b = tile
    const long flops = 2L * g.M * g.N * g.K;
    if (a_bf16) dfx::launch_timed(flops, -5, BM * 1000 + BN, gemm_bf16_kernel<BM, BN, true>, grid, block, 0, st, g);
    else dfx::launch_timed(flops, -5, BM * 1000 + BN, gemm_bf16_kernel<BM, BN, false>, grid, block, 0, st, g);
    return dfx::check_launch("gemm_bf16_kernel");
}

}  // namespace

extern "C" int dfx_gemm_bf16(const void *A, int a_dtype, long lda, const void *W, long ldw, const float *bias, const float *R,
                             long ldr, void *C, int c_dtype, long ldc, int M, int N, int K, int act, void *stream)
{
    if (M < 0 || N < 0 || K <= 0) return dfx::fail(DFX_EINVAL, "gemm_bf16: bad dimension");
    if (a_dtype < 0 || a_dtype > 1 || c_dtype < 0 || c_dtype > 1)
        return dfx::fail(DFX_EINVAL, "gemm_bf16: unknown dtype code (0 = fp32, 1 = bf16)");
    if (act < 0 || act > 2) return dfx::fail(DFX_EINVAL, "gemm_bf16: activation code must be 0 (none), 1 (ReLU) or 2 (GELU)");
    if (K & 7) return dfx::fail(DFX_EINVAL, "gemm_bf16: K must be a multiple of 8");
    if ((long)M * N == 0) return DFX_OK;
    if (!A || !W || !C) return dfx::fail(DFX_EINVAL, "gemm_bf16: null pointer");
    if (lda < K || ldw < K || ldc < N || (R && ldr < N)) return dfx::fail(DFX_EINVAL, "gemm_bf16: a row pitch is shorter than its row");
    const long ea = a_dtype ? 2 : 4, ec = c_dtype ? 2 : 4;
    if (!dfx::aligned16(A) || !dfx::aligned16(W) || (lda * ea & 15) || (ldw * 2 & 15))
        return dfx::fail(DFX_EINVAL, "gemm_bf16: rows of A and W must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(C) & (uintptr_t)(ec - 1)) || (reinterpret_cast<uintptr_t>(bias) & 3u) || (reinterpret_cast<uintptr_t>(R) & 3u))
        return dfx::fail(DFX_EINVAL, "gemm_bf16: C, bias and R must be aligned to their element size");
    if ((long)M * lda * ea >= (1L << 31) || (long)N * ldw * 2 >= (1L << 31) || (long)M * ldc * ec >= (1L << 31) ||
        (R && (long)M * ldr * 4 >= (1L << 31)))
        return dfx::fail(DFX_ERANGE, "gemm_bf16: an operand reaches 2 GiB");
    Args g;
    g.A = A, g.lda = lda;
    g.W = static_cast<const unsigned short *>(W), g.ldw = ldw;
    g.bias = bias;
    g.R = R, g.ldr = ldr;
    g.C = C, g.ldc = ldc, g.c_bf16 = c_dtype;
    g.M = M, g.N = N, g.K = K, g.act = act;
    g.wide = (N & 7) == 0 && dfx::aligned16(C) && (ldc * ec & 15) == 0 && (!R || (dfx::aligned16(R) && (ldr & 3) == 0));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // Tile choice: 128 x 128 (half the operand traffic per flop) once it gives every CU two tiles, 64 x 64 below that - four times
    // the workgroups for the launches of a few hundred to a few thousand rows.
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    if (t128 >= 512) return launch<128, 128>(g, a_dtype, st);
    return launch<64, 64>(g, a_dtype, st);
}
