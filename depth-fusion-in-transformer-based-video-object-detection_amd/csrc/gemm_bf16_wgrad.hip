// Weight gradient of a Linear on the bf16 matrix cores of gfx950 (include/dfx_gemm_bf16.h, dfx_gemm_bf16_wgrad):
//   dW[n][k] = sum_m bf16(dY[m][n]) bf16(X[m][k]),   db[n] = sum_m dY[m][n]   (db from the unrounded fp32 values)
// The bf16 twin of gemm_wgrad.hip: the same output tiles, the same cut of M into row ranges with a partial slab each, the
// same reduction launch (wgrad_reduce.h), the same buffer descriptors of the exact extent of a range.  What differs is the
// operand path.  v_mfma_f32_32x32x16_bf16 wants 8 consecutive indices of the SUMMED dimension per lane, and here the summed
// dimension is the row index m of both operands - the slow one in memory.  So a step of BK = 32 rows is staged as it lies in
// memory, As[r][n] and Bs[r][k] in bf16 (two float4 -> eight bf16, round-to-nearest-even, one ds_write_b128; no bf16 copy of an
// operand reaches memory), and a lane's fragment - 8 consecutive r of ONE column - is two ds_read_b64_tr_b16, gfx950's
// transposed LDS read: per group of 16 lanes a block of 4 rows x 16 columns arrives column-major, lane 4q + p supplying the
// address of row q, columns 4p .. 4p + 3, lane i receiving column i with row q in element q.
//
// What that read needs, and how the kernel gives it:
//   EXEC all ones: the K loop, the staging and the db sum branch on workgroup-uniform values only; tails of M arrive as zeros
//   through the descriptors, columns beyond N / K start from kOut, the tile is padded and nothing is masked;
//   8-byte aligned lane addresses: the row pitch is a multiple of 4 elements and a lane's column a multiple of 4;
//   no swizzle: stores and reads go through the one `lds_off(row, col)` below, plain rows.  The pitch is BM + 32 (BN + 32)
//   elements = 64 bytes beyond a multiple of 256, so the 4 rows x 64 bytes that a 32-lane half reads fall on 64 different banks.
#include "dfx_common.h"
#include "dfx_gemm_bf16.h"
#include "mfma_tile.h"
#include "wgrad_reduce.h"

namespace {

using namespace dfx::mfma;
using dfx::wgrad_reduce_kernel;

struct WgradArgs {
    const float *dY = nullptr, *X = nullptr;
    long ldy = 0, ldx = 0;
    float *out = nullptr;     // dW (one range) or the workspace: range s writes out + s * slab, row pitch ldo
    long ldo = 0, slab = 0;
    float *db = nullptr;      // db (one range) or the workspace's first db row, advancing by slab as well; NULL: not computed
    int M = 0, N = 0, K = 0;
    int kper = 0;             // rows of the summed dimension per range (a multiple of BK)
    int nx = 0, ny = 0;       // tiles along K and N
};

constexpr int BK = 32;        // rows of the summed dimension per step: two 16-deep MFMAs

using i16x4 = __attribute__((ext_vector_type(4))) short;

// element offset of (row, col) in a staged image of pitch LD: the one function stores and transposed reads go through
template <int LD>
__device__ __forceinline__ constexpr int lds_off(int row, int col) { return row * LD + col; }

// 4 consecutive rows of one column per lane (see the head of the file); `p` is the address THIS lane supplies
__device__ __forceinline__ i16x4 read_tr(const unsigned short *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) i16x4 *lds_ptr;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p);
#else
    (void)p;
    return i16x4{};
#endif
}

// rows r0 .. r0 + 7 of column (c0 + the lane's column) as one MFMA operand; `mine` = lds_off(8 half + q, 16 (group & 1) + 4 p)
template <int LD>
__device__ __forceinline__ bf16x8 frag_tr(const unsigned short *img, int mine, int s, int c0)
{
    const i16x4 lo = read_tr(img + mine + lds_off<LD>(s * 16, c0));
    const i16x4 hi = read_tr(img + mine + lds_off<LD>(s * 16 + 4, c0));
    using i16x8 = __attribute__((ext_vector_type(8))) short;
    const i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int BM, int WM, int WN>
__global__ __launch_bounds__(256, BM == 128 ? 3 : 4) void gemm_bf16_wgrad_kernel(const WgradArgs g)
{
    constexpr int BN = 128, NTHR = 256;
    using T = Tile<BM, BN, WM, WN, NTHR>;
    constexpr int MT = T::MT, NT = T::NT;
    constexpr int LDA = BM + 32, LDB = BN + 32;               // bf16 elements per staged row
    constexpr int OA = BM / 8, OB = BN / 8;                   // octets (8 columns: two float4 in, one 16-byte LDS store) per row
    constexpr int A_L = BK * OA / NTHR, B_L = BK * OB / NTHR; // octets per thread and step
    constexpr int NG = NTHR / OA;                             // threads that stage the same column octet of dY
    static_assert(BK * OA % NTHR == 0 && BK * OB % NTHR == 0 && NTHR % OA == 0 && NTHR % OB == 0, "a thread keeps its column octet over loads and steps");
    static_assert(LDA % 8 == 0 && LDB % 8 == 0, "16-byte stores and 8-byte transposed reads stay aligned");
    constexpr int A_SZ = BK * LDA, B_SZ = BK * LDB;           // bf16 elements per stage
    constexpr int STAGE_BYTES = 2 * (A_SZ + B_SZ) * 2, C_BYTES = T::PR * T::LDC * 4;
    constexpr int S_BYTES = STAGE_BYTES > C_BYTES ? STAGE_BYTES : C_BYTES;
    static_assert(NG * BM * 4 <= S_BYTES, "the db partials of the column octets fit the stage buffers");
    // one LDS object: the operand stages, then the db partials, then the epilogue's [64][BN + 4] fp32 transpose buffer
    __shared__ __attribute__((aligned(16))) float smem[S_BYTES / 4];
    unsigned short *const stage = reinterpret_cast<unsigned short *>(smem);
    auto As = [&](int buf) { return stage + buf * A_SZ; };                 // As[buf]: [r][n of dY]
    auto Bs = [&](int buf) { return stage + 2 * A_SZ + buf * B_SZ; };     // Bs[buf]: [r][k of X]

    const int tid = threadIdx.x;
    const Lane l = lane_of<T>(tid);
    // (each XCD walks one contiguous range of tiles: the tiles of a range of rows, which share its operands, meet in one L2)
    const int lin = dfx::xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int bx = lin % g.nx, by = (lin / g.nx) % g.ny, split = lin / (g.nx * g.ny);
    const int m0 = by * BM, n0 = bx * BN;                      // first dW row (a dY column) / dW column (an X column)
    const long r0 = (long)split * g.kper;
    const int rows = g.M - r0 < g.kper ? (int)(g.M - r0) : g.kper;   // >= 1: the host leaves no range empty
    const float *A = g.dY + r0 * g.ldy, *B = g.X + r0 * g.ldx;
    const rsrc_t rsA = buffer(A, ((long)(rows - 1) * g.ldy + g.N) * 4);
    const rsrc_t rsB = buffer(B, ((long)(rows - 1) * g.ldx + g.K) * 4);

    // octet f = tid + i * 256 of a step is row f / OA, columns 8 (f % OA) .. + 7 (N % 8 == 0, K % 8 == 0: inside or outside)
    unsigned va[A_L], vb[B_L];
#pragma unroll
    for (int i = 0; i < A_L; ++i) {
        const int f = tid + i * NTHR, r = f / OA, n = m0 + f % OA * 8;
        va[i] = n < g.N ? ((unsigned)r * (unsigned)g.ldy + (unsigned)n) * 4u : kOut;
    }
#pragma unroll
    for (int i = 0; i < B_L; ++i) {
        const int f = tid + i * NTHR, r = f / OB, k = n0 + f % OB * 8;
        vb[i] = k < g.K ? ((unsigned)r * (unsigned)g.ldx + (unsigned)k) * 4u : kOut;
    }
    const unsigned stepA = (unsigned)BK * (unsigned)g.ldy * 4u, stepB = (unsigned)BK * (unsigned)g.ldx * 4u;

    f32x16 acc[MT][NT] = {};
    f32x4 ra[A_L][2], rb[B_L][2];
    f32x4 dbsum[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const bool with_db = g.db != nullptr && bx == 0;           // workgroup-uniform
    auto load_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < A_L; ++i) {
            ra[i][0] = load4(rsA, va[i]);
            ra[i][1] = load4(rsA, va[i] + 16u);
            va[i] += stepA;
        }
#pragma unroll
        for (int i = 0; i < B_L; ++i) {
            rb[i][0] = load4(rsB, vb[i]);
            rb[i][1] = load4(rsB, vb[i] + 16u);
            vb[i] += stepB;
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_L; ++i) {
            const int f = tid + i * NTHR;
            *reinterpret_cast<u32x4 *>(As(buf) + lds_off<LDA>(f / OA, f % OA * 8)) = pack_bf16x8(ra[i][0], ra[i][1]);
            if (with_db) dbsum[0] += ra[i][0], dbsum[1] += ra[i][1];         // the fp32 values, before the rounding
        }
#pragma unroll
        for (int i = 0; i < B_L; ++i) {
            const int f = tid + i * NTHR;
            *reinterpret_cast<u32x4 *>(Bs(buf) + lds_off<LDB>(f / OB, f % OB * 8)) = pack_bf16x8(rb[i][0], rb[i][1]);
        }
    };

    // the address this lane SUPPLIES to a transposed read, relative to the block's first row and the 32-column tile's first column
    const int lane = tid & 63, gl = lane & 15, q = gl >> 2, p = gl & 3, cb = (lane >> 4 & 1) * 16;
    const int mineA = lds_off<LDA>(l.half * 8 + q, l.wm * T::TM + cb + 4 * p);
    const int mineB = lds_off<LDB>(l.half * 8 + q, l.wn * T::TN + cb + 4 * p);

    const int steps = (rows + BK - 1) / BK;
    load_tiles();
    store_tiles(0);
    __syncthreads();
    for (int t = 0; t < steps; ++t) {                          // (workgroup-uniform: EXEC stays all ones at the reads below)
        const int buf = t & 1;
        if (t + 1 < steps) load_tiles();                       // in flight during the MFMAs below
        bf16x8 af[BK / 16][MT], bf[BK / 16][NT];
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
#pragma unroll
            for (int i = 0; i < MT; ++i) af[s][i] = frag_tr<LDA>(As(buf), mineA, s, i * 32);
#pragma unroll
            for (int j = 0; j < NT; ++j) bf[s][j] = frag_tr<LDB>(Bs(buf), mineB, s, j * 32);
        }
#pragma unroll
        for (int s = 0; s < BK / 16; ++s)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
        if (t + 1 < steps) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // db: the NG threads of a column octet meet in LDS and are added in thread order
    if (with_db) {
        float *mine = &smem[(tid / OA) * BM + tid % OA * 8];
        *reinterpret_cast<f32x4 *>(mine) = dbsum[0];
        *reinterpret_cast<f32x4 *>(mine + 4) = dbsum[1];
        __syncthreads();
        if (tid < BM / 4) {
            f32x4 v = *reinterpret_cast<const f32x4 *>(&smem[tid * 4]);
#pragma unroll
            for (int w = 1; w < NG; ++w) v += *reinterpret_cast<const f32x4 *>(&smem[w * BM + tid * 4]);
            const int n = m0 + tid * 4;
            if (n < g.N) {
                float *d = g.db + (long)split * g.slab + n;
                d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
            }
        }
        __syncthreads();
    }

    Epilogue e;
    e.C = g.out + (long)split * g.slab, e.ldc = g.ldo;
    e.M = g.N, e.N = g.K;
    const f32x4 none[1] = {{0.f, 0.f, 0.f, 0.f}};
    epilogue_lean<T, 0, false, false, false>(smem, acc, l, m0, n0, e, none, false);
}

}  // namespace

extern "C" int dfx_gemm_bf16_wgrad(const float *dY, long ldy, const float *X, long ldx, float *dW, long ldw, float *db,
                                   int M, int N, int K, int splits, float *workspace, void *stream)
{
    if (M < 0 || N < 0 || K < 0 || splits < 1) return dfx::fail(DFX_EINVAL, "gemm_bf16_wgrad: bad dimension");
    if ((long)N * K == 0) return DFX_OK;
    if (!dW || (M > 0 && (!dY || !X))) return dfx::fail(DFX_EINVAL, "gemm_bf16_wgrad: null pointer");
    if ((N & 7) || (K & 7)) return dfx::fail(DFX_EINVAL, "gemm_bf16_wgrad: N and K must be multiples of 8");
    if ((ldy & 3) || (ldx & 3) || (ldw & 3) || ldy < N || ldx < K || ldw < K)
        return dfx::fail(DFX_EINVAL, "gemm_bf16_wgrad: ldy, ldx and ldw must be multiples of 4 that cover a row");
    if (!dfx::aligned16(dY) || !dfx::aligned16(X) || !dfx::aligned16(dW) || !dfx::aligned16(workspace))
        return dfx::fail(DFX_EINVAL, "gemm_bf16_wgrad: dY, X, dW and the workspace must be 16-byte aligned");
    // (row offsets of a tile reach up to 128 rows past N before the hardware range check drops them: they must not wrap)
    if (((long)(N + 128) * ldw + K) * 4 >= (1L << 31)) return dfx::fail(DFX_ERANGE, "gemm_bf16_wgrad: dW exceeds 2 GiB");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long NK = (long)N * K, slab = NK + N;
    const unsigned reduce_blocks = (unsigned)(((NK + N) / 4 + 255) / 256);
    if (M == 0) {      // empty sums: exactly what a call with rows would have written, as zeros
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, st, (const float *)nullptr, 0, slab, NK, N, K, dW, ldw, db);
        return dfx::check_launch("wgrad_reduce_kernel");
    }
    const int kper = ((M + splits - 1) / splits + BK - 1) / BK * BK;        // whole 32-row steps per range ...
    splits = (M + kper - 1) / kper;                                          // ... and no range empty
    if (splits > 65535) return dfx::fail(DFX_ERANGE, "gemm_bf16_wgrad: too many splits");
    // (a lane's offset runs one step and 16 bytes past its range before the hardware range check drops it: it must not wrap)
    if ((long)(kper + BK) * (ldy > ldx ? ldy : ldx) * 4 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "gemm_bf16_wgrad: one range of the summed dimension reaches 2 GiB (use more splits)");
    if (splits > 1 && !workspace) return dfx::fail(DFX_EINVAL, "gemm_bf16_wgrad: more than one range needs a workspace");

    WgradArgs g;
    g.dY = dY, g.ldy = ldy, g.X = X, g.ldx = ldx;
    g.M = M, g.N = N, g.K = K, g.kper = kper;
    if (splits > 1) g.out = workspace, g.ldo = K, g.slab = slab, g.db = db ? workspace + NK : nullptr;
    else g.out = dW, g.ldo = ldw, g.slab = 0, g.db = db;
    const bool narrow = N <= 64;          // one 64-row tile: sampling_offsets / attention_weights of the single-level layers
    g.nx = (K + 127) / 128;
    g.ny = narrow ? 1 : (N + 127) / 128;
    const long total = (long)g.nx * g.ny * splits;
    if (total >= (1L << 31)) return dfx::fail(DFX_ERANGE, "gemm_bf16_wgrad: too many tiles");
    // measurement aid (dfx_profile_*): flops of the launch in the byte field, tag_a = -6, tag_b = ranges
    const long flops = 2L * M * N * K;
    const dim3 grid((unsigned)total), block(256);
    if (narrow) dfx::launch_timed(flops, -6, splits, gemm_bf16_wgrad_kernel<64, 1, 4>, grid, block, 0, st, g);
    else dfx::launch_timed(flops, -6, splits, gemm_bf16_wgrad_kernel<128, 2, 2>, grid, block, 0, st, g);
    int rc = dfx::check_launch("gemm_bf16_wgrad_kernel");
    if (rc != DFX_OK || splits == 1) return rc;
    // (measurement aid: bytes moved by the reduction, tag_a = -7, tag_b = ranges)
    dfx::launch_timed(((long)splits + 1) * slab * 4, -7, splits, wgrad_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, st,
                      (const float *)workspace, splits, slab, NK, N, K, dW, ldw, db);
    return dfx::check_launch("wgrad_reduce_kernel");
}
