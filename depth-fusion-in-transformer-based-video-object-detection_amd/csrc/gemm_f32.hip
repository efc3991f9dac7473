// fp32 GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, 256 FLOP/clk/CU) with
// the fused prologue / epilogues of the deformable-attention path (include/dfx_gemm.h).
//
// Structure (CDNA4, wave64):
//   workgroup = 256 threads = 4 waves laid out WM x WN over a BM x BN output tile; a wave owns
//   (BM/WM) x (BN/WN) = MT x NT MFMA tiles of 32 x 32, i.e. MT*NT*16 accumulator registers per lane
//   (mfma_tile.h: the tile geometry, the K-step over one LDS stage and the epilogues, shared with conv_igemm.hip)
//   K is walked in steps of BK = 16 through a double-buffered LDS stage:
//     As[buf][m][k]  - A (and Linear weights, Bs[buf][n][k]) arrive K-contiguous as 16-byte loads and
//                      are stored as they are, one ds_write_b128 each; row pitch BK+4 floats = five
//                      16-byte slots, so the 16 lanes of a ds_read_b128 group (16 different rows, the
//                      same k) fall on 16 different slots
//     Bs[buf][k][n]  - activations of a 1x1 convolution are already [K][N]: 16-byte LDS stores
//   the next K-step's global loads are issued into registers before the 8 x MT*NT MFMAs of the
//   current step, and written to the other LDS buffer after them: one barrier per K-step
//   epilogue: + bias (per row for convolutions, per column for Linear), + residual, ReLU, zeroing of masked
//   rows; through LDS and out as float4 where C allows it, else straight from the accumulators.
// MFMA-bound: 2*M*N*K flops against 157 TFLOP/s (fp32 matrix peak, MI355X_MICROARCH.md).
#include "dfx_common.h"
#include "dfx_gemm.h"
#include "mfma_tile.h"
#include <stdlib.h>

namespace {

using namespace dfx::mfma;

struct Args {
    const float *A = nullptr, *A2 = nullptr;
    long lda = 0, strideA = 0;
    const float *B = nullptr;
    long ldb = 0, strideB = 0;
    const float *bias = nullptr;
    int bias_per_row = 0;
    const float *R = nullptr;
    long ldr = 0, strideR = 0;
    const unsigned char *mask = nullptr;
    long strideMask = 0;
    float *C = nullptr;
    long ldc = 0, strideC = 0;
    int M = 0, N = 0, K = 0, relu = 0;
    int cblk = 0;             // > 0: C is stored column-block-major, [ceil(N / cblk)][M][cblk] (include/dfx_gemm.h)
    long cblk_stride = 0;     // elements between column blocks (>= M * cblk)
    long ablk_stride = 0;     // > 0: A is K-block-major, [K / 4][M][4] with this many elements between blocks
    int wide_epilogue = 0;    // row-major C (and R) with 16-byte aligned rows, N % 4 == 0: float4 epilogue through LDS
    int splits = 1, kper = 0; // split-K: z = batch * splits + split, split s covers k in [s * kper, min(K, (s + 1) * kper))
    int nx = 0, ny = 0;       // tiles along N and M (the grid is one-dimensional: nx * ny * nz workgroups)
    const float *B2 = nullptr;// two-segment [K,N] operand: rows k >= K1 come from B2 (row k - K1), same ldb; LDS-DMA path only
    long strideB2 = 0;
    int K1 = 0;
    int group_m = 0;          // tile order (placement only, never results): 0 = n fastest, then m, then z, as dispatched;
                              // > 0: workgroup ids are XCD-remapped (each XCD walks one contiguous range) and run m fastest inside
                              // groups of group_m tile rows, then along the columns of every batch element
    int fast_cblk = 0;        // column-block-major C through the same LDS round trip (set by launch())
    int fast_epi = 0;         // wide epilogue in its lean form (set by launch(): no GELU, C and R slices < 2 GiB)
    long strideBias = 0;      // elements the column bias advances per batch element (wide column blocks run as a batch: dfx_gemm_f32)
};

// the product every entry point starts from: C[M,N] = A[M,K] x B, one K range, plain row-major C
Args product(const float *A, long lda, const float *B, long ldb, float *C, long ldc, int M, int N, int K)
{
    Args g;
    g.A = A, g.lda = lda;
    g.B = B, g.ldb = ldb;
    g.C = C, g.ldc = ldc;
    g.M = M, g.N = N, g.K = g.kper = K;
    return g;
}

// waves per SIMD the register allocation must leave room for (HIP's second __launch_bounds__ argument; what the K loop's own
// needs allow: 168 / 120 / 96 / 64 registers per lane for the 128 x 128 / 64 x 128 / 128 x 64 / 64 x 64 tiles, two 8-wave
// workgroups of the 256 x 128 tile; without the bound the scheduler hoists the epilogue's loads over everything and takes
// 2-3x the registers, i.e. a third of the resident waves)
constexpr int min_blocks(int BM, int BN, int NW, int BK)
{
    return BK != 16 ? 1 : NW == 8 ? 4 : BM == 128 && BN == 128 ? 3 : BM == 64 && BN == 128 ? 4
           : BM == 128 && BN == 64 ? 5 : BM == 64 && BN == 64 ? 6 : BM == 128 && BN == 96 ? 3 : BM == 128 && BN == 32 ? 6 : 1;
}

// tile (bx, by) of batch element / split bz that this workgroup computes (scalar arithmetic; see Args::group_m)
__device__ __forceinline__ void tile_coords(const Args &g, int &bx, int &by, long &bz)
{
    int lin = blockIdx.x;
    if (g.group_m > 0) {
        lin = dfx::xcd_remap(lin, (int)gridDim.x);
        const int nJ = (int)(gridDim.x / (unsigned)g.ny);           // columns of all batch elements
        const int grp = lin / (g.group_m * nJ), y0 = grp * g.group_m;
        const int gsz = min(g.ny - y0, g.group_m), r = lin - grp * g.group_m * nJ;
        by = y0 + r % gsz;
        const int J = r / gsz;
        bx = J % g.nx;
        bz = J / g.nx;
    } else {
        bx = lin % g.nx;
        by = (lin / g.nx) % g.ny;
        bz = lin / (g.nx * g.ny);
    }
}

// Column-block-major C ([N / w][M][w], w = 4 or 12: what msda_level_forward reads) through the LDS round trip of the float4
// epilogues: a pass's float4s are numbered block-major - (block, row, quad of the block), quad fastest - so that consecutive
// lanes write consecutive memory (64 rows x w floats of one block per wave-instruction for w = 4) instead of one scattered
// dword per lane and accumulator register.
template <class T>
__device__ __forceinline__ void epilogue_cblk(float *Ct, const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const Epilogue &e)
{
    constexpr int NF4 = T::PR * T::CQ;                     // float4 per pass
    const bool brow = e.bias && e.bias_per_row, bcol = e.bias && !e.bias_per_row;
    const int QB = e.cblk >> 2, b0 = n0 / e.cblk;         // quads per block, first block of the tile
    const __amdgpu_buffer_rsrc_t rsC = buffer(e.C, ((long)(e.N / e.cblk - 1) * e.cblk_stride + (long)e.M * e.cblk) * 4);
#pragma unroll
    for (int p = 0; p < T::BM / T::PR; ++p) {
        if (p > 0) __syncthreads();
        acc_to_lds<T>(Ct, acc, l, p);
        __syncthreads();
#pragma unroll
        for (int e0 = 0; e0 < NF4; e0 += T::NTHR) {
            const int f = e0 + l.tid;
            if (NF4 % T::NTHR != 0 && f >= NF4) break;
            const int blk = f / (T::PR * QB), rem = f - blk * (T::PR * QB), row = rem / QB, sub = rem - row * QB;
            const int m = m0 + T::tile_row(p, row);
            const int q = blk * QB + sub, n = n0 + q * 4;
            f32x4 v = *reinterpret_cast<const f32x4 *>(&Ct[row * T::LDC + q * 4]);
            const bool ok = m < e.M && n < e.N;
            if (bcol) v += *reinterpret_cast<const f32x4 *>(e.bias + min(n, e.N - 4));
            if (brow) v += e.bias[min(m, e.M - 1)];
            if (e.act) relu4(v);
            if (e.mask && e.mask[min(m, e.M - 1)]) v = (f32x4){0.f, 0.f, 0.f, 0.f};
            store4(v, rsC, ok ? (unsigned)(((long)(b0 + blk) * e.cblk_stride + (long)m * e.cblk + sub * 4) * 4) : kOut);
        }
    }
}

template <int BM, int BN, int WM, int WN, bool B_KN, int BK, bool DMA>
__global__ __launch_bounds__(64 * WM * WN, min_blocks(BM, BN, WM * WN, BK)) void gemm_f32_kernel(const Args g)
{
    using T = Tile<BM, BN, WM, WN, 64 * WM * WN>;
    constexpr int MT = T::MT, NT = T::NT;
    constexpr int LDK = BK + 4;                       // [m][k] / [n][k] pitch: 5 (BK = 16) sixteen-byte slots
    constexpr int LDB = T::LDB;                       // [k][n] pitch of the [K][N] operand (16-byte aligned rows)
    constexpr int KQ = BK / 4;                        // float4 per row per K-step
    constexpr int BQ = B_KN ? BN / 4 : KQ;            // ... per row of the staged B image
    constexpr int A_F4 = BM * KQ, B_F4 = BN * KQ;     // float4 per K-step in the A / B tile (= BK * BN / 4 for the [K][N] operand as well)
    constexpr int NW = WM * WN, NTHR = 64 * NW;       // waves / threads of the workgroup (4 / 256, or 8 / 512 for the 256 x 128 tile)
    constexpr int A_LOADS = (A_F4 + NTHR - 1) / NTHR; // ... per thread (last pass may be partial)
    constexpr int B_LOADS = (B_F4 + NTHR - 1) / NTHR;
    static_assert(NW == 4 || NW == 8, "bad wave layout");
    static_assert(BK % 8 == 0, "a ds_read_b128 covers 8 consecutive k (4 per lane half)");
    // one LDS object: the two operand stages, re-used by the epilogues as a [64][BN + 4] transpose buffer
    constexpr int A_SZ = BM * LDK, B_SZ = B_KN ? BK * LDB : BN * LDK;               // floats per stage
    constexpr int C_SZ = T::PR * T::LDC;
    constexpr int S_SZ = 2 * (A_SZ + B_SZ) > C_SZ ? 2 * (A_SZ + B_SZ) : C_SZ;
    __shared__ __attribute__((aligned(16))) float smem[S_SZ];
    float (*const As)[A_SZ] = reinterpret_cast<float (*)[A_SZ]>(smem);              // As[buf]: [m][k]
    float (*const Bs)[B_SZ] = reinterpret_cast<float (*)[B_SZ]>(smem + 2 * A_SZ);   // Bs[buf]: [k][n] or [n][k]

    // ---- tile coordinates and this workgroup's slices of the operands ------------------------------------------------
    const int tid = threadIdx.x, lane = tid & 63;
    const Lane l = lane_of<T>(tid);
    int bx, by;
    long bz;
    tile_coords(g, bx, by, bz);
    const int m0 = by * BM, n0 = bx * BN;
    const long cz = bz;                                   // C slice: one per (batch, split)
    int kbeg = 0, K = g.K;                                // this workgroup's K range
    if (g.splits > 1) {
        const int split = (int)(bz % g.splits);
        bz /= g.splits;
        kbeg = split * g.kper;
        K = min(g.K - kbeg, g.kper);
    }
    const long ashift = g.ablk_stride > 0 ? (long)(kbeg >> 2) * g.ablk_stride : (long)kbeg;
    const float *A = g.A + bz * g.strideA + ashift;
    const float *A2 = g.A2 ? g.A2 + bz * g.strideA + ashift : nullptr;
    const float *B = g.B + bz * g.strideB + (B_KN ? (long)kbeg * g.ldb : (long)kbeg);

    f32x16 acc[MT][NT] = {};

    // ---- operand staging by buffer loads --------------------------------------------------------------------------------
    // One descriptor per operand whose size is the operand's exact extent, a 32-bit byte offset per lane that advances by
    // a constant per K-step; rows / columns outside the problem get kOut (mfma_tile.h; the host checks that an operand
    // stays below 2 GiB).  K tails: rows of a [K][N] operand and blocks of a K-block-major A beyond K lie past the extent
    // as well; for K-contiguous operands the last K-step masks its lanes (wave-uniform branch).
    const long bytesA = g.ablk_stride > 0 ? ((long)(K / 4 - 1) * g.ablk_stride + (long)g.M * 4) * 4
                                          : ((long)(g.M - 1) * g.lda + K) * 4;
    const long bytesB = B_KN ? ((long)(K - 1) * g.ldb + g.N) * 4 : ((long)(g.N - 1) * g.ldb + K) * 4;
    const __amdgpu_buffer_rsrc_t rsA = buffer(A, bytesA), rsA2 = buffer(A2 ? A2 : A, bytesA);
    // (two-segment operand: rsB covers rows 0 .. K1 - 1, rsB2 the rest)
    const __amdgpu_buffer_rsrc_t rsB = buffer(B, (B_KN && g.B2) ? ((long)(g.K1 - 1) * g.ldb + g.N) * 4 : bytesB);
    const __amdgpu_buffer_rsrc_t rsB2 = buffer((B_KN && g.B2) ? g.B2 + bz * g.strideB2 : B, ((long)(g.K - g.K1 - 1) * g.ldb + g.N) * 4);
    // byte offset of float4 kq of tile row `row` of A; of float4 q of row r of the staged B image ([k][n]: r = k, else r = n)
    auto a_off = [&](int row, int kq) {
        const int m = m0 + row;
        const unsigned o = g.ablk_stride > 0 ? ((unsigned)kq * (unsigned)g.ablk_stride + (unsigned)m * 4u) * 4u
                                             : ((unsigned)m * (unsigned)g.lda + (unsigned)kq * 4u) * 4u;
        return m < g.M ? o : kOut;
    };
    auto b_off = [&](int r, int q) {
        const int n = B_KN ? n0 + q * 4 : n0 + r;
        const unsigned o = B_KN ? ((unsigned)r * (unsigned)g.ldb + (unsigned)n) * 4u : ((unsigned)n * (unsigned)g.ldb + (unsigned)q * 4u) * 4u;
        return n < g.N ? o : kOut;
    };
    unsigned va[A_LOADS], vb[B_LOADS];
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
        const int f = tid + i * NTHR;
        va[i] = f < A_F4 ? a_off(f / KQ, f % KQ) : kOut;
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int f = tid + i * NTHR;
        vb[i] = f < B_F4 ? b_off(f / BQ, f % BQ) : kOut;
    }
    const unsigned stepA = g.ablk_stride > 0 ? (unsigned)(BK / 4) * (unsigned)g.ablk_stride * 4u : BK * 4u;
    const unsigned stepB = B_KN ? (unsigned)BK * (unsigned)g.ldb * 4u : BK * 4u;

    f32x4 ra[A_LOADS], ra2[A_LOADS], rb[B_LOADS];
    bool ktail = false;                   // the loaded K-step reaches past K (wave-uniform)
    int ktail_k0 = 0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto load_tiles = [&](int k0) {
        ktail = k0 + BK > K;
        ktail_k0 = k0;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            ra[i] = load4(rsA, va[i]);
            if (A2) ra2[i] = load4(rsA2, va[i]);
            va[i] += stepA;
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            rb[i] = load4(rsB, vb[i]);
            vb[i] += stepB;
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int f = tid + i * NTHR, row = f / KQ, kq = f % KQ;
            if (f >= A_F4) continue;
            f32x4 v = ra[i];
            if (A2) v += ra2[i];
            if (ktail && g.ablk_stride == 0 && ktail_k0 + kq * 4 >= K) v = zero4;
            *reinterpret_cast<f32x4 *>(&As[buf][row * LDK + kq * 4]) = v;
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int f = tid + i * NTHR, r = f / BQ, q = f % BQ;
            if (f >= B_F4) continue;
            f32x4 v = rb[i];
            if (!B_KN && ktail && ktail_k0 + q * 4 >= K) v = zero4;
            *reinterpret_cast<f32x4 *>(&Bs[buf][r * (B_KN ? LDB : LDK) + q * 4]) = v;
        }
    };

    // Residual prefetch (64-row tiles only: 8 float4 per thread): a short K (Bottleneck.conv3: 4-16 K-steps) leaves the
    // epilogue's residual loads nothing to hide behind, so they are issued here, before the K loop, through a buffer
    // descriptor of the residual's exact extent (rows / columns outside the problem return zeros, never used).
    constexpr bool PREFETCH_R = BM == 64 && BN == 128;
    f32x4 rpre[PREFETCH_R ? T::NIT : 1];
    const bool use_rpre = PREFETCH_R && g.R && g.wide_epilogue;
    if (PREFETCH_R && use_rpre) {
        const __amdgpu_buffer_rsrc_t rsR = buffer(g.R + bz * g.strideR, ((long)(g.M - 1) * g.ldr + g.N) * 4);
#pragma unroll
        for (int i = 0; i < T::NIT; ++i) {
            const int f = tid + i * NTHR, m = m0 + f / T::CQ, n = n0 + f % T::CQ * 4;
            rpre[PREFETCH_R ? i : 0] = load4(rsR, (m < g.M && n < g.N) ? ((unsigned)m * (unsigned)g.ldr + (unsigned)n) * 4u : kOut);
        }
    }
    // ---- LDS-DMA staging (DMA = true: no A2 prologue, K a multiple of BK) -------------------------------------------
    // The same LDS images, filled by `buffer_load_dwordx4 ... lds`: the data go from memory straight to LDS, so the
    // VGPR -> LDS store traffic of a K-step (16 KB per workgroup at ~80 B/clk/CU, which delays the other waves' fragment
    // reads: ablation in DESIGN.md, 125 -> 143 TFLOP/s without the stores) disappears, and so do the staging
    // registers.  A wave-instruction fills 64 consecutive 16-byte slots; the images keep their padded pitch (5 slots per
    // K-contiguous row, BN/4 + 1 per [k][n] row), the lane that falls on a pad slot re-loads its neighbour.  Per-lane
    // byte offsets are loop-invariant, the K-step advances through the instruction's scalar offset; rows / columns
    // outside the problem carry an offset beyond the extent and arrive as zeros.
    constexpr int A_SLOTS = BM * (LDK / 4), B_PITCH = B_KN ? LDB / 4 : LDK / 4, B_SLOTS = (B_KN ? BK : BN) * B_PITCH;
    constexpr int A_INSTR = (A_SLOTS + 63) / 64, B_INSTR = (B_SLOTS + 63) / 64;
    constexpr int A_PW = (A_INSTR + NW - 1) / NW, B_PW = (B_INSTR + NW - 1) / NW;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned dva[DMA ? A_PW : 1], dvb[DMA ? B_PW : 1];
    bool dpa[DMA ? A_PW : 1], dpb[DMA ? B_PW : 1];
    if (DMA) {
#pragma unroll
        for (int i = 0; i < A_PW; ++i) {
            const int sl = (wave_u + NW * i) * 64 + lane;
            dpa[i] = wave_u + NW * i < A_INSTR && sl < A_SLOTS;
            dva[i] = a_off(sl / (LDK / 4), min(sl % (LDK / 4), KQ - 1));
        }
#pragma unroll
        for (int i = 0; i < B_PW; ++i) {
            const int sl = (wave_u + NW * i) * 64 + lane;
            dpb[i] = wave_u + NW * i < B_INSTR && sl < B_SLOTS;
            dvb[i] = b_off(sl / B_PITCH, min(sl % B_PITCH, BQ - 1));
        }
    }
    auto dma_tiles = [&](int k0, int buf) {
        const unsigned sa = g.ablk_stride > 0 ? (unsigned)(k0 >> 2) * (unsigned)g.ablk_stride * 4u : (unsigned)k0 * 4u;
        const bool second = B_KN && g.B2 && k0 >= g.K1;             // (scalar: a K-step lies in one segment, K1 % BK == 0)
        const unsigned sb = B_KN ? (unsigned)(second ? k0 - g.K1 : k0) * (unsigned)g.ldb * 4u : (unsigned)k0 * 4u;
#pragma unroll
        for (int i = 0; i < A_PW; ++i)
            if (dpa[i]) lds_dma16(rsA, As[buf] + (wave_u + NW * i) * 256, dva[i], sa);
        if (second) {
#pragma unroll
            for (int i = 0; i < B_PW; ++i)
                if (dpb[i]) lds_dma16(rsB2, Bs[buf] + (wave_u + NW * i) * 256, dvb[i], sb);
        } else {
#pragma unroll
            for (int i = 0; i < B_PW; ++i)
                if (dpb[i]) lds_dma16(rsB, Bs[buf] + (wave_u + NW * i) * 256, dvb[i], sb);
        }
    };

    // ---- K loop -----------------------------------------------------------------------------------------------------------
    const int steps = (K + BK - 1) / BK;
    if (DMA) {
        dma_tiles(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        load_tiles(0);
        store_tiles(0);
    }
    __syncthreads();
    for (int t = 0; t < steps; ++t) {
        const int buf = t & 1;
        if (!DMA && t + 1 < steps) load_tiles((t + 1) * BK);   // in flight during the MFMAs below
        if constexpr (B_KN && !DMA) kstep_kn<T, BK>(As[buf], Bs[buf], l, acc);
        else kstep_up_front<T, BK, B_KN>(As[buf], Bs[buf], l, acc, [&] { if (DMA && t + 1 < steps) dma_tiles((t + 1) * BK, buf ^ 1); });
        if (!DMA && t + 1 < steps) store_tiles(buf ^ 1);
        if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next tile have landed ...
        __syncthreads();                                        // ... and after the barrier so have everybody's
    }

    // ---- epilogue dispatch (mfma_tile.h) ----------------------------------------------------------------------------------
    // (the lane's coordinates are taken from the thread id again: the ones above would otherwise stay in registers through the K
    // loop for the epilogue's sake, and the 256 x 128 tile with a K tail has none to spare)
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const Lane le = lane_of<T>(tid_e);
    Epilogue e;
    e.C = g.C + cz * g.strideC, e.ldc = g.ldc;
    e.R = g.R ? g.R + bz * g.strideR : nullptr, e.ldr = g.ldr;
    e.bias = g.bias ? g.bias + bz * g.strideBias : nullptr, e.bias_per_row = g.bias_per_row;
    e.mask = g.mask ? g.mask + bz * g.strideMask : nullptr;
    e.M = g.M, e.N = g.N, e.act = g.relu;
    e.cblk = g.cblk, e.cblk_stride = g.cblk_stride;
    if constexpr (T::LEAN) if (g.wide_epilogue && g.fast_epi) return epilogue_lean_any<T, PREFETCH_R>(smem, acc, le, m0, n0, e, rpre, use_rpre);
    if (g.cblk > 0 && g.fast_cblk) return epilogue_cblk<T>(smem, acc, le, m0, n0, e);      // (launch(): ReLU or no activation)
    if (g.wide_epilogue) return epilogue_float4<T, PREFETCH_R>(smem, acc, le, m0, n0, e, rpre, use_rpre);
    epilogue_scalar<T>(acc, le, m0, n0, e);
}

// Tile order of a launch (Args::group_m, read from DFX_GEMM_GROUP): every XCD walks one contiguous range of tiles, 8 tile rows at
// a time with the row fastest, so that the workgroups resident on an XCD share few operand panels in its 4 MiB L2.  Measured at 32 frames
// (tools/bench_gemm.py, DFX_GEMM_GROUP = 0 / 1 / 2 / 4 / 8 / 16 / all rows in one process each, profiles/r03_gemm_order.txt):
// 4 and 8 tie, 2.7 % less time over the path's shapes than the dispatch order (layer4 shortcut 4 %, layer2 conv3 6 %).
template <int BM, int BN, int WM, int WN, int BK = 16>
int launch(const Args &g_in, int batch, int b_is_kn, hipStream_t st)
{
    Args g = g_in;
    g.nx = (g.N + BN - 1) / BN;
    g.ny = (g.M + BM - 1) / BM;
    const long total = (long)g.nx * g.ny * batch * (g.splits > 1 ? g.splits : 1);
    if (total >= (1L << 31)) return dfx::fail(DFX_ERANGE, "gemm: too many tiles");
    g.group_m = dfx::tuning().gemm_group;
    g.fast_cblk = g.cblk > 0 && g.cblk % 4 == 0 && BN % g.cblk == 0 && g.N % g.cblk == 0 && !g.R && g.relu != 2 &&
                  (!g.bias || g.bias_per_row || dfx::aligned16(g.bias)) && dfx::aligned16(g.C) && (g.cblk_stride & 3) == 0 && (g.strideC & 3) == 0 &&
                  ((long)(g.N / g.cblk) * g.cblk_stride) * 4 < (1L << 31);
    // (row offsets of a tile reach up to BM rows past M before the hardware range check drops them: they must not wrap)
    g.fast_epi = g.wide_epilogue && g.relu != 2 && ((long)(g.M + BM) * g.ldc + g.N) * 4 < (1L << 31) &&
                 (!g.R || ((long)(g.M + BM) * g.ldr + g.N) * 4 < (1L << 31));
    const dim3 grid((unsigned)total), block(64 * WM * WN);
    // measurement aid (dfx_profile_*): flops of the launch in the byte field, tag_a = -1 ([K,N] operand: 1x1 convolution)
    // or -2 (Linear), tag_b = tile
    const long flops = 2L * g.M * g.N * g.K * batch;
    const int kloc = g.splits > 1 ? g.kper : g.K;
    // LDS-DMA staging unless the prologue add needs registers, K has a tail, or the kernel is the HBM-bound short-K
    // residual convolution (layer1 / layer2 conv3), where the DMA wait also drains the residual prefetch
    bool dma = !g.A2 && g.K % BK == 0 && kloc % BK == 0 && !(g.R && kloc <= 128) && !dfx::tuning().gemm_no_dma;
    if (g.B2) {
        if (g.A2 || g.K % BK || g.K1 % BK || g.splits > 1 || !b_is_kn)
            return dfx::fail(DFX_EINVAL, "gemm: a two-segment operand needs K and K1 multiples of %d, no A2, no split-K", BK);
        dma = true;
    }
    if (dma) {
        if (b_is_kn) dfx::launch_timed(flops, -1, BM * 1000 + BN, gemm_f32_kernel<BM, BN, WM, WN, true, BK, true>, grid, block, 0, st, g);
        else dfx::launch_timed(flops, -2, BM * 1000 + BN, gemm_f32_kernel<BM, BN, WM, WN, false, BK, true>, grid, block, 0, st, g);
    } else {
        if (b_is_kn) dfx::launch_timed(flops, -1, BM * 1000 + BN, gemm_f32_kernel<BM, BN, WM, WN, true, BK, false>, grid, block, 0, st, g);
        else dfx::launch_timed(flops, -2, BM * 1000 + BN, gemm_f32_kernel<BM, BN, WM, WN, false, BK, false>, grid, block, 0, st, g);
    }
    return dfx::check_launch("gemm_f32_kernel");
}

// ---- Linears over few rows (the 300-query layers: M = 300 x frames of the rank, N and K a few hundred) ----------------------
// A 64 x 64 tile leaves such a product 76-600 workgroups, each a chain of K / 2 dependent MFMAs per wave behind one memory
// round trip (K = 256: 3.7 us of MFMAs + ~2 us of latency, whatever the tile: profiles/r03_temporal_timeline_F4.txt).  Here a
// workgroup owns ONE 32 x 32 tile of C and its NW waves split K: wave w sums k in [w K/NW, (w+1) K/NW) in chunks of 64, every
// lane loading the 128 contiguous bytes of "its" row of A and of W per chunk straight into the MFMA operand registers (the
// MFMA sums over k in any order as long as A and B agree: lane (c, h) feeds step 4j + t of a chunk with k = 32h + 4j + t) -
// no LDS staging, no K loop barrier, all loads of the wave in flight at once - and the NW partial tiles meet in LDS.
// Same products and the same per-output k order within a wave; the cross-wave sum adds NW partials in wave order.
template <int NW, int CH>
__global__ __launch_bounds__(64 * NW) void linear_rows_kernel(const Args g)
{
    __shared__ __attribute__((aligned(16))) float red[NW][32][36];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int bx = blockIdx.x % g.nx, by = blockIdx.x / g.nx;
    const int m0 = by * 32, n0 = bx * 32;
    const __amdgpu_buffer_rsrc_t rsA = buffer(g.A, ((long)(g.M - 1) * g.lda + g.K) * 4);
    const __amdgpu_buffer_rsrc_t rsA2 = buffer(g.A2 ? g.A2 : g.A, ((long)(g.M - 1) * g.lda + g.K) * 4);
    const __amdgpu_buffer_rsrc_t rsB = buffer(g.B, ((long)(g.N - 1) * g.ldb + g.K) * 4);
    const int kw = wave * (CH * 64) + 32 * h;                      // first k of this lane in chunk 0
    const unsigned oa = m0 + c < g.M ? ((unsigned)(m0 + c) * (unsigned)g.lda + (unsigned)kw) * 4u : kOut;
    const unsigned ob = n0 + c < g.N ? ((unsigned)(n0 + c) * (unsigned)g.ldb + (unsigned)kw) * 4u : kOut;
    f32x4 a[CH][8], b[CH][8];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a[ch][j] = load4(rsA, oa, (ch * 64 + j * 4) * 4);
            b[ch][j] = load4(rsB, ob, (ch * 64 + j * 4) * 4);
        }
    if (g.A2) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                a[ch][j] += load4(rsA2, oa, (ch * 64 + j * 4) * 4);
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][j][t], b[ch][j][t], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][acc_row(r, h)][c] = acc[r];
    __syncthreads();
    if (tid < 256) {
        const int row = tid >> 3, c4 = (tid & 7) * 4;
        const int m = m0 + row, n = n0 + c4;
        if (m < g.M && n < g.N) {
            float4 v = *reinterpret_cast<const float4 *>(&red[0][row][c4]);
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                const float4 q = *reinterpret_cast<const float4 *>(&red[w][row][c4]);
                v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
            }
            if (g.wide_epilogue && n + 3 < g.N) {
                if (g.bias) { const float4 q = *reinterpret_cast<const float4 *>(g.bias + n); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
                if (g.R) { const float4 q = *reinterpret_cast<const float4 *>(g.R + (long)m * g.ldr + n); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
                if (g.relu) { v.x = activate(v.x, g.relu); v.y = activate(v.y, g.relu); v.z = activate(v.z, g.relu); v.w = activate(v.w, g.relu); }
                *reinterpret_cast<float4 *>(g.C + (long)m * g.ldc + n) = v;
            } else {                                           // narrow heads (class / box / reference-point Linears: N = 2 .. 4)
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (n + u >= g.N) break;
                    float x = e[u] + (g.bias ? g.bias[n + u] : 0.f);
                    if (g.R) x += g.R[(long)m * g.ldr + n + u];
                    if (g.relu) x = activate(x, g.relu);
                    g.C[(long)m * g.ldc + n + u] = x;
                }
            }
        }
    }
}

// few rows, [N,K] operand, plain row-major operands and epilogue: K = 64 * NW * CH
bool rows_kernel_applies(const Args &g, int batch, int b_is_kn)
{
    const int max_rows = dfx::tuning().gemm_rows_max;          // tuning aid: the row limit (0 = kernel off)
    const int tiles_n = (g.N + 31) / 32;
    return !b_is_kn && batch == 1 && g.splits <= 1 && !g.mask && !g.cblk && !g.ablk_stride && !g.B2 &&
           !g.bias_per_row && (g.M <= max_rows || (max_rows > 0 && g.N <= 128)) && (g.N <= 32 || (g.N % 32 == 0 && g.wide_epilogue)) && g.N <= 1024 &&
           (g.K == 256 || g.K == 512 || g.K == 1024) && (long)((g.M + 31) / 32) * tiles_n <= 9600;
}

int launch_rows(const Args &g_in, hipStream_t st)
{
    Args g = g_in;
    g.nx = (g.N + 31) / 32;
    g.ny = (g.M + 31) / 32;
    const dim3 grid((unsigned)(g.nx * g.ny));
    const long flops = 2L * g.M * g.N * g.K;
    if (g.K == 256) dfx::launch_timed(flops, -2, 32032, linear_rows_kernel<4, 1>, grid, dim3(256), 0, st, g);
    else if (g.K == 512) dfx::launch_timed(flops, -2, 32032, linear_rows_kernel<8, 1>, grid, dim3(512), 0, st, g);
    else dfx::launch_timed(flops, -2, 32032, linear_rows_kernel<8, 2>, grid, dim3(512), 0, st, g);
    return dfx::check_launch("linear_rows_kernel");
}

int choose_and_launch(const Args &g, int batch, int b_is_kn, hipStream_t st);

}  // namespace

extern "C" int dfx_gemm_f32(const float *A, const float *A2, long lda, long strideA, const float *B, long ldb,
                            long strideB, int b_is_kn, const float *bias, int bias_per_row, const float *R,
                            long ldr, long strideR, const unsigned char *row_mask, long strideMask, float *C,
                            long ldc, long strideC, int M, int N, int K, int batch, int relu, int c_block,
                            long c_block_stride, long a_block_stride, void *stream)
{
    if (M < 0 || N < 0 || K <= 0 || batch < 0) return dfx::fail(DFX_EINVAL, "gemm: bad dimension");
    if (relu < 0 || relu > 2) return dfx::fail(DFX_EINVAL, "gemm: activation code must be 0 (none), 1 (ReLU) or 2 (GELU)");
    if ((long)M * N * batch == 0) return DFX_OK;
    if (!A || !B || !C) return dfx::fail(DFX_EINVAL, "gemm: null pointer");
    if ((K & 3) || (lda & 3) || (ldb & 3) || (strideA & 3) || (strideB & 3) || !dfx::aligned16(A) || !dfx::aligned16(B) ||
        (A2 && !dfx::aligned16(A2)) || (b_is_kn && (N & 3)))
        return dfx::fail(DFX_EINVAL, "gemm: K (and N for [K,N] operands) must be multiples of 4, rows 16-byte aligned");
    if (batch > 65535) return dfx::fail(DFX_ERANGE, "gemm: batch too large");
    {   // 32-bit byte offsets inside one batch element's operands (buffer loads)
        const long ea = a_block_stride > 0 ? (long)(K / 4) * a_block_stride : (long)M * lda;
        const long eb = b_is_kn ? (long)K * ldb : (long)N * ldb;
        if (ea * 4 >= (1L << 31) || eb * 4 >= (1L << 31) || (R && (long)M * ldr * 4 >= (1L << 31)))
            return dfx::fail(DFX_ERANGE, "gemm: an operand exceeds 2 GiB per batch element");
    }
    if (c_block < 0 || (c_block > 0 && (c_block_stride < (long)M * c_block || R)))
        return dfx::fail(DFX_EINVAL, "gemm: column-block-major C needs c_block_stride >= M * c_block and no residual");
    if (a_block_stride < 0 || (a_block_stride > 0 && (a_block_stride < (long)M * 4 || (a_block_stride & 3) || A2)))
        return dfx::fail(DFX_EINVAL, "gemm: K-block-major A needs a_block_stride >= 4 * M (a multiple of 4) and no A2");
    if (c_block >= 128 && c_block % 128 == 0 && N % c_block == 0 && N > c_block && batch == 1 && !b_is_kn && !R && a_block_stride == 0 &&
        (c_block_stride & 3) == 0 && dfx::aligned16(C) && (!bias || bias_per_row || dfx::aligned16(bias))) {
        // Wide column blocks ([N / w][M][w] with w a multiple of the tile width: Linears that share their input, stacked along
        // N, each result a contiguous [M, w] tensor of its own - the decoder layers' value projections): every block is a
        // product of its own on the same A.  They run as ONE launch over the batch axis - A fixed, W / the column bias / C
        // advancing per block - in the XCD-aware tile order, which walks the columns of ALL blocks for a group of tile rows
        // before it moves on: an A panel is read once for the whole stack.
        Args g = product(A, lda, B, ldb, C, c_block, M, c_block, K);
        g.A2 = A2;
        g.strideB = (long)c_block * ldb, g.strideC = c_block_stride;
        g.bias = bias, g.bias_per_row = bias_per_row, g.strideBias = bias_per_row ? 0 : c_block;
        g.mask = row_mask;
        g.relu = relu, g.wide_epilogue = 1;
        return choose_and_launch(g, N / c_block, 0, static_cast<hipStream_t>(stream));
    }
    const int wide = c_block == 0 && (N & 3) == 0 && (ldc & 3) == 0 && (strideC & 3) == 0 && dfx::aligned16(C) &&
                     (!R || ((ldr & 3) == 0 && (strideR & 3) == 0 && dfx::aligned16(R))) &&
                     (!bias || bias_per_row || dfx::aligned16(bias));
    Args g = product(A, lda, B, ldb, C, ldc, M, N, K);
    g.A2 = A2;
    g.strideA = strideA, g.strideB = strideB, g.strideC = strideC;
    g.bias = bias, g.bias_per_row = bias_per_row;
    g.R = R, g.ldr = ldr, g.strideR = strideR;
    g.mask = row_mask, g.strideMask = strideMask;
    g.relu = relu, g.wide_epilogue = wide;
    g.cblk = c_block, g.cblk_stride = c_block_stride, g.ablk_stride = a_block_stride;
    return choose_and_launch(g, batch, b_is_kn, static_cast<hipStream_t>(stream));
}

// Y[n] = act(W x [X1[n]; X2[n]] + bias): the last 1x1 convolution of a bottleneck and its stride-1 projection shortcut in
// ONE product over the concatenated input channels (include/dfx_gemm.h)
extern "C" int dfx_conv1x1_pair_f32(const float *W, const float *X1, long strideX1, int K1, const float *X2, long strideX2,
                                    int K2, const float *bias, float *Y, long strideY, int Co, int HW, int batch, int act,
                                    void *stream)
{
    if (Co < 0 || HW < 0 || K1 <= 0 || K2 <= 0 || batch < 0) return dfx::fail(DFX_EINVAL, "conv1x1_pair: bad dimension");
    if (act < 0 || act > 2) return dfx::fail(DFX_EINVAL, "conv1x1_pair: activation code must be 0, 1 or 2");
    if ((long)Co * HW * batch == 0) return DFX_OK;
    if (!W || !X1 || !X2 || !Y) return dfx::fail(DFX_EINVAL, "conv1x1_pair: null pointer");
    const int K = K1 + K2;
    if ((K1 & 15) || (K2 & 15) || (HW & 3) || (strideX1 & 3) || (strideX2 & 3) || (strideY & 3) || !dfx::aligned16(W) ||
        !dfx::aligned16(X1) || !dfx::aligned16(X2) || !dfx::aligned16(Y))
        return dfx::fail(DFX_EINVAL, "conv1x1_pair: channel counts must be multiples of 16, H*W of 4, buffers 16-byte aligned");
    if (batch > 65535 || (long)Co * K * 4 >= (1L << 31) || (long)K1 * HW * 4 >= (1L << 31) || (long)K2 * HW * 4 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "conv1x1_pair: an operand exceeds 2 GiB per image");
    Args g = product(W, K, X1, HW, Y, HW, Co, HW, K);
    g.strideB = strideX1, g.strideC = strideY;
    g.B2 = X2, g.strideB2 = strideX2, g.K1 = K1;
    g.bias = bias, g.bias_per_row = 1;
    g.relu = act, g.wide_epilogue = 1;
    return choose_and_launch(g, batch, 1, static_cast<hipStream_t>(stream));
}

namespace {

int choose_and_launch(const Args &g, int batch, int b_is_kn, hipStream_t st)
{
    const int M = g.M, N = g.N, K = g.splits > 1 ? g.kper : g.K;
    const long zb = (long)batch * (g.splits > 1 ? g.splits : 1);
    if (rows_kernel_applies(g, batch, b_is_kn)) return launch_rows(g, st);
    // tile choice.  Small M / N pick the matching narrow tile.
    switch (dfx::tuning().gemm_tile) {       // tuning aid (DFX_GEMM_TILE): force one tile for every launch
    case 0: return launch<128, 128, 2, 2>(g, batch, b_is_kn, st);
    case 1: return launch<128, 64, 2, 2>(g, batch, b_is_kn, st);
    case 2: return launch<64, 128, 1, 4>(g, batch, b_is_kn, st);
    case 5: return launch<64, 64, 2, 2>(g, batch, b_is_kn, st);
    case 6: return launch<64, 64, 2, 2, 64>(g, batch, b_is_kn, st);
    case 7: return launch<256, 128, 4, 2>(g, batch, b_is_kn, st);
    default: break;
    }
    if (M <= 64) return launch<64, 128, 1, 4>(g, batch, b_is_kn, st);
    if (N <= 32) return launch<128, 32, 4, 1>(g, batch, b_is_kn, st);
    if (N <= 64) return launch<128, 64, 2, 2>(g, batch, b_is_kn, st);
    if (N <= 96) return launch<128, 96, 4, 1>(g, batch, b_is_kn, st);
    // Measured on the path's shapes at 32 frames (tools/bench_gemm.py with DFX_GEMM_TILE, profiles/r02_bench_gemm_tiles.txt):
    // the 128 x 128 tile (half the operand traffic per flop) is 2-6 % ahead wherever it still gives every CU several
    // tiles and K is deep enough to amortise its longer prologue / epilogue; a short K with a residual epilogue
    // (Bottleneck.conv3 of layer2 / layer3) and M = 64 (layer1) stay on 64 x 128 (6 waves per SIMD).
    {
        const long t128x128 = (long)((M + 127) / 128) * ((N + 127) / 128) * zb;
        const bool rows_fit = (M % 128 == 0) || M >= 1024;
        // split-K launches are sized by the caller to fill one resident round of 128 x 128 tiles (3 per CU)
        if (g.splits > 1 && M >= 128 && N >= 128 && t128x128 <= 768) return launch<128, 128, 2, 2>(g, batch, b_is_kn, st);
        // 8 waves on a 256 x 128 tile (two workgroups = 4 waves per SIMD, a quarter fewer LDS-DMA pieces per MFMA): 2-3 % ahead of
        // 128 x 128 on the 2048-channel convolutions of layer4 and behind it everywhere else (profiles/r03_gemm_tile256.txt:
        // ffn2 +10 %, layer3 +9-11 %, layer4 conv1 +4 %, the short-K shapes far worse)
        if (b_is_kn && M % 256 == 0 && M >= 2048 && K >= 512 && t128x128 >= 8192 && g.splits <= 1)
            return launch<256, 128, 4, 2>(g, batch, b_is_kn, st);
        // the same convolutions on the 4- or 8-frame block of a rank (2112 / 4224 tiles of 128 x 128): 128 x 64 - twice the
        // workgroups, more of them resident - is 14-22 % ahead of 256 x 128 and 5-11 % ahead of 128 x 128 at 4 frames, 4-8 % at 8
        // (tools/r03_exp9.sh, profiles/r03_gemm_tiles_F4_F8.txt)
        if (b_is_kn && M % 128 == 0 && M >= 2048 && K >= 512 && K <= 1536 && t128x128 >= 2048 && g.splits <= 1)
            return launch<128, 64, 2, 2>(g, batch, b_is_kn, st);
        // (since the lean epilogue - residual on its way while the tile crosses LDS - the short-K convolutions with a residual
        // take the 128 x 128 tile too once there are 16 tiles per CU: layer1 / layer2 / layer3 conv3 6.6 / 6.9 / 4.5 % faster at
        // 32 frames, layer1 conv3 10 % at 4 and 8; so do the 256 -> 256 Linears: profiles/r03_gemm_tiles_lean_epilogue.txt)
        if (rows_fit && t128x128 >= 2048 && (K >= 512 || (K >= 256 && !g.R && N >= 256) || (b_is_kn && t128x128 >= 4096)))
            return launch<128, 128, 2, 2>(g, batch, b_is_kn, st);
    }
    // Few tiles (token GEMMs of a 4- or 8-frame rank block): all workgroups are resident at once, the CUs that get
    // one tile more than the others set the time.  A 64 x 64 tile halves that quantum (M = 16800, N = 256:
    // 526 tiles of 64 x 128 = 3 on some CUs, 2.05 on average; 1052 of 64 x 64 = 5 against 4.1).
    auto fill = [](long tiles) { return (double)tiles / (256.0 * (double)((tiles + 255) / 256)); };
    const long t128 = (long)((M + 63) / 64) * ((N + 127) / 128) * zb, t64 = (long)((M + 63) / 64) * ((N + 63) / 64) * zb;
    // At most one 64 x 64 workgroup per CU (the 300-query layers of a small rank block: M = 1200, N = 256): nothing hides
    // the global-load latency of a K-step but the step before it, so the K loop runs at ~1 us per step whatever its
    // depth; 64-deep steps quarter their number (profiles/r02_rank_step.txt).
    if (t64 <= 320 && K >= 128) return launch<64, 64, 2, 2, 64>(g, batch, b_is_kn, st);
    // deep 1x1 convolutions of an 8-frame block (layer4 conv1 2048 -> 512, layer2 conv1 512 -> 128): 128 x 64 once it gives
    // every CU 8 tiles, 4-5 % ahead of 64 x 64 / 64 x 128 there (profiles/r03_gemm_tiles_F4_F8.txt)
    if (b_is_kn && M % 128 == 0 && K >= 512 && g.splits <= 1 && (long)(M / 128) * ((N + 63) / 64) * zb >= 2048)
        return launch<128, 64, 2, 2>(g, batch, b_is_kn, st);
    // the decoder's first FFN Linear at 32 frames (9600 x 1024 x 256): 1200 tiles of 128 x 64 are 10 % ahead of 64 x 128 / 64 x 64
    // (tools/bench_gemm_queries.py, tools/r03_exp19.sh: 55.6 vs 61.2 / 57.2 us)
    if (!b_is_kn && M % 128 == 0 && N >= 1024 && K <= 256 && g.splits <= 1 && (long)(M / 128) * ((N + 63) / 64) * zb >= 1024)
        return launch<128, 64, 2, 2>(g, batch, b_is_kn, st);
    if (t128 < 8 * 256 && 0.95 * fill(t64) > fill(t128)) return launch<64, 64, 2, 2>(g, batch, b_is_kn, st);
    return launch<64, 128, 1, 4>(g, batch, b_is_kn, st);
}

// ---- split-K ------------------------------------------------------------------------------------------
// out = act(sum_s ws[s] + bias (+ R)), float4 per thread
__global__ void splitk_reduce_kernel(const float *ws, int splits, long MN, int N, const float *bias, int bias_per_row,
                                     const float *R, long ldr, int act, float *C, long ldc)
{
    const long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i4 * 4 >= MN) return;
    const long e = i4 * 4;
    const int m = (int)(e / N), n = (int)(e - (long)m * N);
    float4 v = *reinterpret_cast<const float4 *>(ws + e);
    for (int s = 1; s < splits; ++s) {
        const float4 q = *reinterpret_cast<const float4 *>(ws + (long)s * MN + e);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    if (bias) {
        if (bias_per_row) { const float b = bias[m]; v.x += b; v.y += b; v.z += b; v.w += b; }
        else { v.x += bias[n]; v.y += bias[n + 1]; v.z += bias[n + 2]; v.w += bias[n + 3]; }
    }
    if (R) { const float *r = R + (long)m * ldr + n; v.x += r[0]; v.y += r[1]; v.z += r[2]; v.w += r[3]; }
    if (act) { v.x = activate(v.x, act); v.y = activate(v.y, act); v.z = activate(v.z, act); v.w = activate(v.w, act); }
    float *c = C + (long)m * ldc + n;
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
}

}  // namespace

extern "C" int dfx_gemm_splitk_f32(const float *A, long lda, const float *B, long ldb, int b_is_kn, const float *bias,
                                   int bias_per_row, const float *R, long ldr, float *C, long ldc, int M, int N, int K,
                                   int act, int splits, float *workspace, void *stream)
{
    if (M < 0 || N < 0 || K <= 0 || splits < 1) return dfx::fail(DFX_EINVAL, "gemm_splitk: bad dimension");
    if (act < 0 || act > 2) return dfx::fail(DFX_EINVAL, "gemm_splitk: activation code must be 0 (none), 1 (ReLU) or 2 (GELU)");
    if ((long)M * N == 0) return DFX_OK;
    if (!A || !B || !C || !workspace) return dfx::fail(DFX_EINVAL, "gemm_splitk: null pointer");
    if ((K & 3) || (N & 3) || (lda & 3) || (ldb & 3) || !dfx::aligned16(A) || !dfx::aligned16(B) || !dfx::aligned16(workspace))
        return dfx::fail(DFX_EINVAL, "gemm_splitk: K and N must be multiples of 4, rows and the workspace 16-byte aligned");
    if ((long)M * lda * 4 >= (1L << 31) || (long)(b_is_kn ? K : N) * ldb * 4 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "gemm_splitk: an operand exceeds 2 GiB");
    int kper = ((K + splits - 1) / splits + 15) / 16 * 16;          // whole K-steps per split
    splits = (K + kper - 1) / kper;
    if (splits > 65535) return dfx::fail(DFX_ERANGE, "gemm_splitk: too many splits");
    Args g = product(A, lda, B, ldb, workspace, N, M, N, K);
    g.strideC = (long)M * N;                                       // one workspace slice per split
    g.wide_epilogue = 1;
    g.splits = splits, g.kper = kper;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = choose_and_launch(g, 1, b_is_kn, st);
    if (rc != DFX_OK) return rc;
    const long quads = ((long)M * N + 3) / 4;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, workspace, splits,
                       (long)M * N, N, bias, bias_per_row, R, ldr, act, C, ldc);
    return dfx::check_launch("splitk_reduce_kernel");
}

// dW[Co,Ci] = sum_n sum_p dZ[n,Co,p] X[n,Ci,p]: the weight gradient of a 1x1 convolution (include/dfx_gemm.h).  Per image it is
// the [M,K] x [N,K]^T product above with the pixels as K, so the images ride the batch axis of the split-K launch: slice
// z = image * splits + range writes slab z, and the reduction adds the slabs in that (ascending) order.
extern "C" int dfx_conv1x1_wgrad_f32(const float *dZ, long strideZ, const float *X, long strideX, float *dW, int Co, int Ci,
                                     int HW, int batch, int splits, float *workspace, void *stream)
{
    if (Co < 0 || Ci < 0 || HW < 0 || batch < 0 || splits < 1) return dfx::fail(DFX_EINVAL, "conv1x1_wgrad: bad dimension");
    if ((long)Co * Ci == 0) return DFX_OK;
    if (!dW || ((long)batch * HW > 0 && (!dZ || !X))) return dfx::fail(DFX_EINVAL, "conv1x1_wgrad: null pointer");
    if ((Co & 3) || (Ci & 3) || (HW & 3) || (strideZ & 3) || (strideX & 3) || !dfx::aligned16(dZ) || !dfx::aligned16(X) ||
        !dfx::aligned16(dW) || !dfx::aligned16(workspace))
        return dfx::fail(DFX_EINVAL, "conv1x1_wgrad: Co, Ci, H*W and the image strides must be multiples of 4, buffers 16-byte aligned");
    if ((long)Co * HW * 4 >= (1L << 31) || (long)Ci * HW * 4 >= (1L << 31) || (long)Co * Ci * 4 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "conv1x1_wgrad: an operand exceeds 2 GiB per image");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((long)batch * HW == 0) {           // empty sums
        if (hipMemsetAsync(dW, 0, (size_t)Co * Ci * 4, st) != hipSuccess) return dfx::fail(DFX_ELAUNCH, "conv1x1_wgrad: memset failed");
        return DFX_OK;
    }
    const int kper = ((HW + splits - 1) / splits + 15) / 16 * 16;      // whole 16-deep steps per range ...
    splits = (HW + kper - 1) / kper;                                    // ... and no range empty
    const long slabs = (long)batch * splits;
    if (slabs > 65535) return dfx::fail(DFX_ERANGE, "conv1x1_wgrad: too many images x ranges");
    if (slabs > 1 && !workspace) return dfx::fail(DFX_EINVAL, "conv1x1_wgrad: more than one image or range needs a workspace");
    Args g = product(dZ, HW, X, HW, slabs > 1 ? workspace : dW, Ci, Co, Ci, HW);
    g.strideA = strideZ, g.strideB = strideX;
    g.strideC = (long)Co * Ci;                                         // one slab per (image, range)
    g.wide_epilogue = 1;
    g.splits = splits, g.kper = kper;
    const int rc = choose_and_launch(g, batch, 0, st);
    if (rc != DFX_OK || slabs == 1) return rc;
    const long quads = (long)Co * Ci / 4;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, workspace, (int)slabs,
                       (long)Co * Ci, Ci, (const float *)nullptr, 0, (const float *)nullptr, 0L, 0, dW, (long)Ci);
    return dfx::check_launch("splitk_reduce_kernel");
}
