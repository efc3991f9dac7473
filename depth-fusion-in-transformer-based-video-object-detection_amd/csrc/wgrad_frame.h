// The frame of the weight-gradient kernels of a Linear, written once (gemm_wgrad.hip: fp32; gemm_bf16_wgrad.hip: bf16 products):
//   dW[n][k] = sum_m dY[m][n] X[m][k],   db[n] = sum_m dY[m][n]
// As a GEMM the output is [N, K] and the summed dimension is the row count M of both operands, so BOTH arrive k-major: a step
// of BK rows is staged as it lies in memory, As[r][n] and Bs[r][k].  Tile geometry, accumulator layout and the lean epilogue are
// the shared ones of mfma_tile.h.
//
// The output has 4-32 tiles while M is frames x 4200, so M is cut into `splits` ranges of whole BK-row steps (the arithmetic
// of dfx_gemm_splitk_f32); every range is a workgroup of its own per tile that writes a partial [N, K] slab (and, tile
// column 0 only, a partial db row behind it) to the workspace, and one reduction launch adds the slabs in ascending order:
// no atomics, the same bits every time.
//
// Addressing: one buffer descriptor per operand of the exact extent of the workgroup's own row range (its base is 64-bit
// pointer arithmetic on the host-checked range size); rows beyond the range fall past the extent and read zeros, columns
// beyond N / K start from kOut - the tail of the summed dimension needs no masking code.  Every branch around the staging, the
// K loop and the db sum is on workgroup-uniform values, so EXEC is all ones wherever a path's K-step reads LDS.
//
// An operand path (`P` below) supplies what differs between the precisions:
//   NAME, KERNEL, TAG    the entry's and the kernel's name in error texts; the dfx_profile_* tag of the product launch (the
//                        reduction's is TAG - 1), or 0: the launches are not timed
//   BK, G, REACH         rows per step; columns of a staged granule (G / 4 float4 loads, one LDS store); rows beyond a range
//                        that the 2 GiB bound of a range allows for
//   elem, pitch(cols)    the element of an LDS image and its row pitch in elements
//   put(dst, v)          one granule, as loaded, to its place in an LDS image
//   Frags<T>             the per-lane set-up of the K-step and kstep(As, Bs, l, acc) over one staged step
#pragma once
#include <hip/hip_runtime.h>
#include "dfx_common.h"
#include "mfma_tile.h"

namespace dfx {
namespace {

using namespace mfma;

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

// element offset of (row, col) in a staged image of pitch LD: the one function the stores and a path's reads go through
template <int LD>
__device__ __forceinline__ constexpr int lds_off(int row, int col) { return row * LD + col; }

template <class P, int BM, int WM, int WN>
__global__ __launch_bounds__(256, BM == 128 ? 3 : 4) void gemm_wgrad_kernel(const WgradArgs g)
{
    constexpr int BN = 128, NTHR = 256;
    using T = Tile<BM, BN, WM, WN, NTHR>;
    using E = typename P::elem;
    constexpr int MT = T::MT, NT = T::NT;
    constexpr int BK = P::BK, G = P::G, H = G / 4;             // a granule: G columns of one row, H float4 in flight
    constexpr int LDA = P::pitch(BM), LDB = P::pitch(BN);
    constexpr int QA = BM / G, QB = BN / G;                    // granules per staged row
    constexpr int A_L = BK * QA / NTHR, B_L = BK * QB / NTHR;  // granules per thread and step
    constexpr int NG = NTHR / QA;                              // threads that stage the same column granule of dY
    static_assert(BK * QA % NTHR == 0 && BK * QB % NTHR == 0 && NTHR % QA == 0 && NTHR % QB == 0, "a thread keeps its column granule over loads and steps");
    static_assert(LDA * sizeof(E) % 16 == 0 && LDB * sizeof(E) % 16 == 0 && G * sizeof(E) % 16 == 0, "the 16-byte LDS stores stay aligned");
    constexpr int A_SZ = BK * LDA, B_SZ = BK * LDB;            // elements per stage
    constexpr int STAGE_BYTES = 2 * (A_SZ + B_SZ) * (int)sizeof(E), C_BYTES = T::PR * T::LDC * 4;
    constexpr int S_BYTES = STAGE_BYTES > C_BYTES ? STAGE_BYTES : C_BYTES;
    static_assert(NG * BM * 4 <= S_BYTES, "the db partials of the column granules fit the stage buffers");
    // one LDS object: the operand stages, then the db partials, then the epilogue's [64][BN + 4] fp32 transpose buffer
    __shared__ __attribute__((aligned(16))) float smem[S_BYTES / 4];
    E *const stage = reinterpret_cast<E *>(smem);
    auto As = [&](int buf) { return stage + buf * A_SZ; };                 // As[buf]: [r][n of dY]
    auto Bs = [&](int buf) { return stage + 2 * A_SZ + buf * B_SZ; };     // Bs[buf]: [r][k of X]

    const int tid = threadIdx.x;
    const Lane l = lane_of<T>(tid);
    // (each XCD walks one contiguous range of tiles: the tiles of a range of rows, which share its operands, meet in one L2)
    const int lin = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int bx = lin % g.nx, by = (lin / g.nx) % g.ny, split = lin / (g.nx * g.ny);
    const int m0 = by * BM, n0 = bx * BN;                      // first dW row (a dY column) / dW column (an X column)
    const long r0 = (long)split * g.kper;
    const int rows = g.M - r0 < g.kper ? (int)(g.M - r0) : g.kper;   // >= 1: the host leaves no range empty
    const float *A = g.dY + r0 * g.ldy, *B = g.X + r0 * g.ldx;
    const rsrc_t rsA = buffer(A, ((long)(rows - 1) * g.ldy + g.N) * 4);
    const rsrc_t rsB = buffer(B, ((long)(rows - 1) * g.ldx + g.K) * 4);

    // granule f = tid + i * 256 of a step is row f / QA, columns G (f % QA) .. + G - 1 (N % G == 0, K % G == 0: inside or outside)
    unsigned va[A_L], vb[B_L];
#pragma unroll
    for (int i = 0; i < A_L; ++i) {
        const int f = tid + i * NTHR, r = f / QA, n = m0 + f % QA * G;
        va[i] = n < g.N ? ((unsigned)r * (unsigned)g.ldy + (unsigned)n) * 4u : kOut;
    }
#pragma unroll
    for (int i = 0; i < B_L; ++i) {
        const int f = tid + i * NTHR, r = f / QB, k = n0 + f % QB * G;
        vb[i] = k < g.K ? ((unsigned)r * (unsigned)g.ldx + (unsigned)k) * 4u : kOut;
    }
    const unsigned stepA = (unsigned)BK * (unsigned)g.ldy * 4u, stepB = (unsigned)BK * (unsigned)g.ldx * 4u;

    f32x16 acc[MT][NT] = {};
    f32x4 ra[A_L][H], rb[B_L][H];                              // the step in flight
    f32x4 dbsum[H] = {};
    const bool with_db = g.db != nullptr && bx == 0;           // workgroup-uniform
    auto load_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < A_L; ++i) {
#pragma unroll
            for (int h = 0; h < H; ++h) ra[i][h] = load4(rsA, va[i] + 16u * h);
            va[i] += stepA;
        }
#pragma unroll
        for (int i = 0; i < B_L; ++i) {
#pragma unroll
            for (int h = 0; h < H; ++h) rb[i][h] = load4(rsB, vb[i] + 16u * h);
            vb[i] += stepB;
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_L; ++i) {
            const int f = tid + i * NTHR;
            P::put(As(buf) + lds_off<LDA>(f / QA, f % QA * G), ra[i]);
            if (with_db) {                                     // the fp32 values as loaded: before any rounding of a path
#pragma unroll
                for (int h = 0; h < H; ++h) dbsum[h] += ra[i][h];
            }
        }
#pragma unroll
        for (int i = 0; i < B_L; ++i) {
            const int f = tid + i * NTHR;
            P::put(Bs(buf) + lds_off<LDB>(f / QB, f % QB * G), rb[i]);
        }
    };
    const typename P::template Frags<T> frags(l);

    const int steps = (rows + BK - 1) / BK;
    load_tiles();
    store_tiles(0);
    __syncthreads();
    for (int t = 0; t < steps; ++t) {                          // (workgroup-uniform, as is `t + 1 < steps`)
        const int buf = t & 1;
        if (t + 1 < steps) load_tiles();                       // in flight during the MFMAs below
        frags.kstep(As(buf), Bs(buf), l, acc);
        if (t + 1 < steps) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // db: the NG threads of a column granule meet in LDS and are added in thread order
    if (with_db) {
        float *mine = &smem[(tid / QA) * BM + tid % QA * G];
#pragma unroll
        for (int h = 0; h < H; ++h) *reinterpret_cast<f32x4 *>(mine + 4 * h) = dbsum[h];
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

// The reduction launch: every range of the summed dimension left a partial [N, K] slab and, behind it, a partial db row in the
// workspace.  dW = sum_s slab_s, db = sum_s db row_s, ascending s (splits = 0: zeros); float4 per thread, the db quads follow
// the dW quads
__global__ void wgrad_reduce_kernel(const float *ws, int splits, long slab, long NK, int N, int K, float *dW, long ldw, float *db)
{
    const long e = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    float *dst;
    if (e < NK) {
        const long n = e / K;
        dst = dW + n * ldw + (e - n * K);
    } else if (db && e < NK + N) {
        dst = db + (e - NK);
    } else {
        return;
    }
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (splits > 0) v = *reinterpret_cast<const f32x4 *>(ws + e);
    for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const f32x4 *>(ws + (long)s * slab + e);
    dst[0] = v[0], dst[1] = v[1], dst[2] = v[2], dst[3] = v[3];
}

// (measurement aid, dfx_profile_*: a path with a TAG stamps its launches - `bytes`, tag_a = tag, tag_b = ranges; TAG 0 does not)
template <class P, class Kernel, class... Args>
inline void wgrad_launch(long bytes, int tag, int ranges, Kernel kernel, unsigned blocks, hipStream_t st, Args... args)
{
    if (P::TAG) launch_timed(bytes, tag, ranges, kernel, dim3(blocks), dim3(256), 0, st, args...);
    else hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, args...);
}

// The body of both extern "C" entries (include/dfx_gemm.h dfx_gemm_wgrad_f32, include/dfx_gemm_bf16.h dfx_gemm_bf16_wgrad)
template <class P>
int wgrad_entry(const float *dY, long ldy, const float *X, long ldx, float *dW, long ldw, float *db, int M, int N, int K, int splits,
                float *workspace, void *stream)
{
    constexpr int BK = P::BK, G = P::G;
    if (M < 0 || N < 0 || K < 0 || splits < 1) return fail(DFX_EINVAL, "%s: bad dimension", P::NAME);
    if ((long)N * K == 0) return DFX_OK;
    if (!dW || (M > 0 && (!dY || !X))) return fail(DFX_EINVAL, "%s: null pointer", P::NAME);
    if (N % G || K % G) return fail(DFX_EINVAL, "%s: N and K must be multiples of %d", P::NAME, G);
    if ((ldy & 3) || (ldx & 3) || (ldw & 3) || ldy < N || ldx < K || ldw < K)
        return fail(DFX_EINVAL, "%s: ldy, ldx and ldw must be multiples of 4 that cover a row", P::NAME);
    if (!aligned16(dY) || !aligned16(X) || !aligned16(dW) || !aligned16(workspace))
        return fail(DFX_EINVAL, "%s: dY, X, dW and the workspace must be 16-byte aligned", P::NAME);
    // (row offsets of a tile reach up to 128 rows past N before the hardware range check drops them: they must not wrap)
    if (((long)(N + 128) * ldw + K) * 4 >= (1L << 31)) return fail(DFX_ERANGE, "%s: dW exceeds 2 GiB", P::NAME);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long NK = (long)N * K, slab = NK + N;
    const unsigned reduce_blocks = (unsigned)(((NK + N) / 4 + 255) / 256);
    if (M == 0) {      // empty sums: exactly what a call with rows would have written, as zeros
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, st, (const float *)nullptr, 0, slab, NK, N, K, dW, ldw, db);
        return check_launch("wgrad_reduce_kernel");
    }
    const int kper = ((M + splits - 1) / splits + BK - 1) / BK * BK;        // whole BK-row steps per range ...
    splits = (M + kper - 1) / kper;                                          // ... and no range empty
    if (splits > 65535) return fail(DFX_ERANGE, "%s: too many splits", P::NAME);
    // A lane's 32-bit offset must not wrap while the hardware range check still has to drop it.  Both paths advance the offset by
    // one step after every load, the last one included, but that last value is never used: the largest offset a load uses lies
    // inside the kper rows of the range, and the fp32 path (REACH = 0) bounds exactly those.  The bf16 path addresses the second
    // float4 of an octet 16 bytes past the offset, and its bound was stated with a whole step of room (REACH = BK) so that even
    // the advanced offset plus those 16 bytes stays below 2^31; each entry keeps the bound, and the wording, it has had.
    if ((long)(kper + P::REACH) * (ldy > ldx ? ldy : ldx) * 4 >= (1L << 31))
        return fail(DFX_ERANGE, "%s: one range of the summed dimension %s 2 GiB (use more splits)", P::NAME, P::REACH ? "reaches" : "exceeds");
    if (splits > 1 && !workspace) return fail(DFX_EINVAL, "%s: more than one range needs a workspace", P::NAME);

    WgradArgs g;
    g.dY = dY, g.ldy = ldy, g.X = X, g.ldx = ldx;
    g.M = M, g.N = N, g.K = K, g.kper = kper;
    if (splits > 1) g.out = workspace, g.ldo = K, g.slab = slab, g.db = db ? workspace + NK : nullptr;
    else g.out = dW, g.ldo = ldw, g.slab = 0, g.db = db;
    const bool narrow = N <= 64;          // one 64-row tile: sampling_offsets / attention_weights of the single-level layers
    g.nx = (K + 127) / 128;
    g.ny = narrow ? 1 : (N + 127) / 128;
    const long total = (long)g.nx * g.ny * splits;
    if (total >= (1L << 31)) return fail(DFX_ERANGE, "%s: too many tiles", P::NAME);
    const long flops = 2L * M * N * K;
    if (narrow) wgrad_launch<P>(flops, P::TAG, splits, gemm_wgrad_kernel<P, 64, 1, 4>, (unsigned)total, st, g);
    else wgrad_launch<P>(flops, P::TAG, splits, gemm_wgrad_kernel<P, 128, 2, 2>, (unsigned)total, st, g);
    int rc = check_launch(P::KERNEL);
    if (rc != DFX_OK || splits == 1) return rc;
    wgrad_launch<P>(((long)splits + 1) * slab * 4, P::TAG - 1, splits, wgrad_reduce_kernel, reduce_blocks, st, (const float *)workspace,
                    splits, slab, NK, N, K, dW, ldw, db);
    return check_launch("wgrad_reduce_kernel");
}

}  // namespace
}  // namespace dfx
