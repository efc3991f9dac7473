// Weight gradient of a Linear on the gfx950 matrix cores (include/dfx_gemm.h, dfx_gemm_wgrad_f32):
//   dW[n][k] = sum_m dY[m][n] X[m][k],   db[n] = sum_m dY[m][n]
// As a GEMM the output is [N, K] and the summed dimension is the row count M of both operands, so BOTH arrive k-major:
// a K-step of 16 rows is staged as it lies in memory, As[r][n] (pitch BM + 4) and Bs[r][k] (pitch LDB), one ds_write_b128
// per 16-byte load, and a lane's fragment of either operand is one ds_read_b32 per MFMA - the access kstep_kn (mfma_tile.h)
// makes for its [K,N] operand, here for A as well.  Tile geometry, accumulator layout and the lean epilogue are the shared ones.
//
// The output has 4-32 tiles while M is frames x 4200, so M is cut into `splits` ranges of whole 16-row steps (the arithmetic
// of dfx_gemm_splitk_f32); every range is a workgroup of its own per tile that writes a partial [N, K] slab (and, tile
// column 0 only, a partial db row behind it) to the workspace, and one reduction launch adds the slabs in ascending order:
// no atomics, the same bits every time.
//
// Addressing: one buffer descriptor per operand of the exact extent of the workgroup's own row range (its base is 64-bit
// pointer arithmetic on the host-checked range size); rows beyond the range fall past the extent and read zeros, columns
// beyond N / K start from kOut - the tail of the summed dimension needs no masking code.
#include "dfx_common.h"
#include "dfx_gemm.h"
#include "mfma_tile.h"
#include "wgrad_reduce.h"

namespace {

using namespace dfx::mfma;
using dfx::wgrad_reduce_kernel;      // (wgrad_reduce.h: shared with gemm_bf16_wgrad.hip)

struct WgradArgs {
    const float *dY = nullptr, *X = nullptr;
    long ldy = 0, ldx = 0;
    float *out = nullptr;     // dW (one range) or the workspace: range s writes out + s * slab, row pitch ldo
    long ldo = 0, slab = 0;
    float *db = nullptr;      // db (one range) or the workspace's first db row, advancing by slab as well; NULL: not computed
    int M = 0, N = 0, K = 0;
    int kper = 0;             // rows of the summed dimension per range (a multiple of 16)
    int nx = 0, ny = 0;       // tiles along K and N
};

constexpr int BK = 16;

// [k][m] x [k][n]: both fragments by ds_read_b32 (their rows run along m / n), one MFMA group ahead of the MFMAs
template <class T, int LDA>
__device__ __forceinline__ void kstep_km_kn(const float *As, const float *Bs, const Lane &l, f32x16 (&acc)[T::MT][T::NT])
{
    float a[2][T::MT], b[2][T::NT];
#pragma unroll
    for (int i = 0; i < T::MT; ++i) a[0][i] = As[frag_k(0, l.half) * LDA + l.wm * T::TM + i * 32 + l.c];
#pragma unroll
    for (int j = 0; j < T::NT; ++j) b[0][j] = Bs[frag_k(0, l.half) * T::LDB + l.wn * T::TN + j * 32 + l.c];
#pragma unroll
    for (int q = 0; q < BK / 2; ++q) {
        if (q + 1 < BK / 2) {
#pragma unroll
            for (int i = 0; i < T::MT; ++i) a[(q + 1) & 1][i] = As[frag_k(q + 1, l.half) * LDA + l.wm * T::TM + i * 32 + l.c];
#pragma unroll
            for (int j = 0; j < T::NT; ++j) b[(q + 1) & 1][j] = Bs[frag_k(q + 1, l.half) * T::LDB + l.wn * T::TN + j * 32 + l.c];
        }
        __builtin_amdgcn_sched_barrier(0);      // (as in kstep_kn: the next group's reads stay ahead of this group's MFMAs)
#pragma unroll
        for (int i = 0; i < T::MT; ++i)
#pragma unroll
            for (int j = 0; j < T::NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q & 1][i], b[q & 1][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int BM, int WM, int WN>
__global__ __launch_bounds__(256, BM == 128 ? 3 : 4) void gemm_wgrad_kernel(const WgradArgs g)
{
    constexpr int BN = 128, NTHR = 256;
    using T = Tile<BM, BN, WM, WN, NTHR>;
    constexpr int MT = T::MT, NT = T::NT;
    constexpr int LDA = BM + 4, LDB = T::LDB;
    constexpr int QA = BM / 4, QB = BN / 4;                    // float4 per staged row
    constexpr int A_F4 = BK * QA, B_F4 = BK * QB;
    constexpr int A_LOADS = A_F4 / NTHR, B_LOADS = B_F4 / NTHR;
    constexpr int NG = NTHR / QA;                              // threads that stage the same column quad of dY
    static_assert(A_F4 % NTHR == 0 && B_F4 % NTHR == 0 && NTHR % QA == 0, "a thread keeps its column quad over loads and K-steps");
    constexpr int A_SZ = BK * LDA, B_SZ = BK * LDB, C_SZ = T::PR * T::LDC;
    constexpr int S_SZ = 2 * (A_SZ + B_SZ) > C_SZ ? 2 * (A_SZ + B_SZ) : C_SZ;
    static_assert(NG * BM <= S_SZ, "the db partials of the column quads fit the stage buffers");
    __shared__ __attribute__((aligned(16))) float smem[S_SZ];
    float (*const As)[A_SZ] = reinterpret_cast<float (*)[A_SZ]>(smem);              // As[buf]: [r][n of dY]
    float (*const Bs)[B_SZ] = reinterpret_cast<float (*)[B_SZ]>(smem + 2 * A_SZ);   // Bs[buf]: [r][k of X]

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

    unsigned va[A_LOADS], vb[B_LOADS];
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
        const int f = tid + i * NTHR, r = f / QA, n = m0 + f % QA * 4;
        va[i] = n < g.N ? ((unsigned)r * (unsigned)g.ldy + (unsigned)n) * 4u : kOut;
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int f = tid + i * NTHR, r = f / QB, k = n0 + f % QB * 4;
        vb[i] = k < g.K ? ((unsigned)r * (unsigned)g.ldx + (unsigned)k) * 4u : kOut;
    }
    const unsigned stepA = (unsigned)BK * (unsigned)g.ldy * 4u, stepB = (unsigned)BK * (unsigned)g.ldx * 4u;

    f32x16 acc[MT][NT] = {};
    f32x4 ra[A_LOADS], rb[B_LOADS];
    f32x4 dbsum = {0.f, 0.f, 0.f, 0.f};
    const bool with_db = g.db != nullptr && bx == 0;           // workgroup-uniform
    auto load_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            ra[i] = load4(rsA, va[i]);
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
            const int f = tid + i * NTHR;
            *reinterpret_cast<f32x4 *>(&As[buf][(f / QA) * LDA + f % QA * 4]) = ra[i];
            if (with_db) dbsum += ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int f = tid + i * NTHR;
            *reinterpret_cast<f32x4 *>(&Bs[buf][(f / QB) * LDB + f % QB * 4]) = rb[i];
        }
    };

    const int steps = (rows + BK - 1) / BK;
    load_tiles();
    store_tiles(0);
    __syncthreads();
    for (int t = 0; t < steps; ++t) {
        const int buf = t & 1;
        if (t + 1 < steps) load_tiles();                       // in flight during the MFMAs below
        kstep_km_kn<T, LDA>(As[buf], Bs[buf], l, acc);
        if (t + 1 < steps) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // db: the NG threads of a column quad meet in LDS and are added in thread order
    if (with_db) {
        *reinterpret_cast<f32x4 *>(&smem[(tid / QA) * BM + tid % QA * 4]) = dbsum;
        __syncthreads();
        if (tid < QA) {
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

extern "C" int dfx_gemm_wgrad_f32(const float *dY, long ldy, const float *X, long ldx, float *dW, long ldw, float *db,
                                  int M, int N, int K, int splits, float *workspace, void *stream)
{
    if (M < 0 || N < 0 || K < 0 || splits < 1) return dfx::fail(DFX_EINVAL, "gemm_wgrad: bad dimension");
    if ((long)N * K == 0) return DFX_OK;
    if (!dW || (M > 0 && (!dY || !X))) return dfx::fail(DFX_EINVAL, "gemm_wgrad: null pointer");
    if ((N & 3) || (K & 3)) return dfx::fail(DFX_EINVAL, "gemm_wgrad: N and K must be multiples of 4");
    if ((ldy & 3) || (ldx & 3) || (ldw & 3) || ldy < N || ldx < K || ldw < K)
        return dfx::fail(DFX_EINVAL, "gemm_wgrad: ldy, ldx and ldw must be multiples of 4 that cover a row");
    if (!dfx::aligned16(dY) || !dfx::aligned16(X) || !dfx::aligned16(dW) || !dfx::aligned16(workspace))
        return dfx::fail(DFX_EINVAL, "gemm_wgrad: dY, X, dW and the workspace must be 16-byte aligned");
    // (row offsets of a tile reach up to 128 rows past N before the hardware range check drops them: they must not wrap)
    if (((long)(N + 128) * ldw + K) * 4 >= (1L << 31)) return dfx::fail(DFX_ERANGE, "gemm_wgrad: dW exceeds 2 GiB");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long NK = (long)N * K, slab = NK + N;
    const unsigned reduce_blocks = (unsigned)(((NK + N) / 4 + 255) / 256);
    if (M == 0) {      // empty sums: exactly what a call with rows would have written, as zeros
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, st, (const float *)nullptr, 0, slab, NK, N, K, dW, ldw, db);
        return dfx::check_launch("wgrad_reduce_kernel");
    }
    const int kper = ((M + splits - 1) / splits + BK - 1) / BK * BK;        // whole 16-row steps per range ...
    splits = (M + kper - 1) / kper;                                          // ... and no range empty
    if (splits > 65535) return dfx::fail(DFX_ERANGE, "gemm_wgrad: too many splits");
    if ((long)kper * (ldy > ldx ? ldy : ldx) * 4 >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "gemm_wgrad: one range of the summed dimension exceeds 2 GiB (use more splits)");
    if (splits > 1 && !workspace) return dfx::fail(DFX_EINVAL, "gemm_wgrad: more than one range needs a workspace");

    WgradArgs g;
    g.dY = dY, g.ldy = ldy, g.X = X, g.ldx = ldx;
    g.M = M, g.N = N, g.K = K, g.kper = kper;
    if (splits > 1) g.out = workspace, g.ldo = K, g.slab = slab, g.db = db ? workspace + NK : nullptr;
    else g.out = dW, g.ldo = ldw, g.slab = 0, g.db = db;
    const bool narrow = N <= 64;          // one 64-row tile: sampling_offsets / attention_weights of the single-level layers
    g.nx = (K + 127) / 128;
    g.ny = narrow ? 1 : (N + 127) / 128;
    const long total = (long)g.nx * g.ny * splits;
    if (total >= (1L << 31)) return dfx::fail(DFX_ERANGE, "gemm_wgrad: too many tiles");
    if (narrow) hipLaunchKernelGGL((gemm_wgrad_kernel<64, 1, 4>), dim3((unsigned)total), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((gemm_wgrad_kernel<128, 2, 2>), dim3((unsigned)total), dim3(256), 0, st, g);
    int rc = dfx::check_launch("gemm_wgrad_kernel");
    if (rc != DFX_OK || splits == 1) return rc;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, st, (const float *)workspace, splits, slab, NK, N, K, dW, ldw, db);
    return dfx::check_launch("wgrad_reduce_kernel");
}
