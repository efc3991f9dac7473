// A bottleneck's last 1x1 convolution and the NEXT block's first one in one launch (include/dfx_gemm.h,
// dfx_conv1x1_chain_f32):
//   Y[n] = relu(W3 x [X1[n] ; X2[n]?] + b3 + R[n]?)     [Co, HW]   written once
//   Z[n] = act(W1 x Y[n] + b1)                          [C1, HW]   from the Y tile while it is still in registers
// The Co-channel map is HBM-bound to write (layer1 / layer2 of ResNet-50: K = 64 / 128 against Co = 256 / 512) and the
// standalone successor reads all of it back only to reduce it to C1 channels; here that read never happens and the
// second product runs on matrix units the first one leaves idle.
//
// Structure (CDNA4, wave64, v_mfma_f32_32x32x2_f32):
//   workgroup = 4 waves = 128 pixels of one frame; a wave owns 32 pixels and ALL channels of them.
//   X: the wave's [K, 32] activation panel lives in registers for the whole kernel, already in MFMA operand form: lane
//      (pixel c = l & 31, half h = l >> 5) holds X[8j + 4h + t][c] as operand of MFMA q = 4j + t - the k numbering of
//      gemm_f32_kernel - loaded as 2 rows x 128 contiguous bytes per instruction.  Nothing of X crosses LDS.
//   Co is walked in tiles of 32 channels.  Per tile the workgroup stages one slab in LDS (fetched into registers under the
//      second product of the tile before, written between two barriers): W3[32 rows of the tile][K] and W1[C1][the tile's 32 columns], both read back as ds_read_b128 A fragments
//      (pitch K + 4 / 36 floats: an odd number of 16-byte slots, so the 16 rows of a read group fall on 16 slots).
//   first product: K / 2 MFMAs into ONE 16-register accumulator (a dependent 32x32x2 chain issues at the full rate),
//      k ascending exactly as gemm_f32_kernel walks it, then + bias, + residual, ReLU in that order: Y is bit-equal to
//      dfx_gemm_f32 / dfx_conv1x1_pair_f32 on the same operands.
//   second product: the accumulator layout (lane = column, register r = row acc_row(r, h)) IS the B-operand
//      layout of k = 8j + 4h + t with r = 4j + t, so register r of the finished Y tile feeds MFMA r of the tile against
//      the natural-order W1 fragment: 16 MFMAs per 32 output channels of Z, no lane movement, no LDS round trip.  A wave
//      sums Z over all Co in ascending k pairs - the order of the standalone GEMM - so Z is bit-equal to it as well.
//   pixels beyond HW carry buffer offsets past every extent: loads return zeros, stores are dropped.
// Channel counts that are no multiple of the instantiated panel (K < 32 KT, C1 < 32 C1T) are zero-filled by the same
// range checks: exact zeros on both operands of the surplus MFMAs.
#include "dfx_common.h"
#include "dfx_gemm.h"
#include "mfma_tile.h"

namespace {

using namespace dfx::mfma;

struct ChainArgs {
    const float *W3, *X1, *X2, *b3, *R, *W1, *b1;
    float *Y, *Z;
    long strideX1, strideX2, strideR, strideY, strideZ;
    int K1, K;            // channels of X1, of both segments
    int Co, C1, HW, relu_z;
    int nx;               // 128-pixel tiles per frame
};

// workgroups per CU the registers must leave room for (256 threads: one wave per SIMD and workgroup)
constexpr int chain_blocks(int KT, int C1T) { return C1T >= 8 ? 1 : KT <= 2 && C1T <= 2 ? 3 : 2; }

template <int KT, int C1T>
__global__ __launch_bounds__(256, chain_blocks(KT, C1T)) void conv1x1_chain_kernel(const ChainArgs g)
{
    constexpr int KP = KT * 32 + 4, W3_SZ = 32 * KP;          // W3 slab [32][KP]
    constexpr int W1P = 36, W1_SZ = C1T * 32 * W1P;           // W1 slab [32 C1T][36]
    constexpr int SLAB = W3_SZ + W1_SZ;
    constexpr int KQ = KT * 8;                                // float4 per W3 slab row
    constexpr int L3 = KT, L1 = C1T;                          // float4 per thread and slab: 32 KQ / 256, 32 C1T 8 / 256
    __shared__ __attribute__((aligned(16))) float smem[SLAB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int bx = blockIdx.x % g.nx;
    const long bz = blockIdx.x / g.nx;
    const int n = bx * 128 + wave * 32 + c;
    const bool ncol = n < g.HW;
    const unsigned HW = (unsigned)g.HW, K = (unsigned)g.K, Co = (unsigned)g.Co;
    const int K2 = g.K - g.K1;

    // a missing operand gets an empty extent: its loads return zeros (x + 0 is exact)
    const __amdgpu_buffer_rsrc_t rsX1 = buffer(g.X1 + bz * g.strideX1, (long)g.K1 * g.HW * 4);
    const __amdgpu_buffer_rsrc_t rsX2 = buffer(g.X2 ? g.X2 + bz * g.strideX2 : g.X1, g.X2 ? (long)K2 * g.HW * 4 : 0);
    const __amdgpu_buffer_rsrc_t rsW3 = buffer(g.W3, (long)g.Co * g.K * 4);
    const __amdgpu_buffer_rsrc_t rsW1 = buffer(g.W1, (long)g.C1 * g.Co * 4);
    const __amdgpu_buffer_rsrc_t rsB3 = buffer(g.b3 ? g.b3 : g.W3, g.b3 ? (long)g.Co * 4 : 0);
    const __amdgpu_buffer_rsrc_t rsB1 = buffer(g.b1 ? g.b1 : g.W1, g.b1 ? (long)g.C1 * 4 : 0);
    const __amdgpu_buffer_rsrc_t rsR = buffer(g.R ? g.R + bz * g.strideR : g.W3, g.R ? (long)g.Co * g.HW * 4 : 0);
    const __amdgpu_buffer_rsrc_t rsY = buffer(g.Y + bz * g.strideY, (long)g.Co * g.HW * 4);
    const __amdgpu_buffer_rsrc_t rsZ = buffer(g.Z + bz * g.strideZ, (long)g.C1 * g.HW * 4);

    // ---- the wave's activation panel: operand q = 4j + t of lane (c, h) is X[8j + 4h + t][n] ----
    float xr[KT * 16];
    const unsigned ncol4 = ncol ? (unsigned)n * 4u : kOut;
#pragma unroll
    for (int q = 0; q < KT * 16; ++q) {
        const int j = q >> 2, t = q & 3, k = 8 * j + 4 * h + t;
        const bool first = 8 * j < g.K1;                           // (scalar: K1 is a multiple of 8; rows beyond K fall past the extent)
        const unsigned kk = first ? (unsigned)k : (unsigned)(k - g.K1);
        xr[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(first ? rsX1 : rsX2, kk * HW * 4u + ncol4, 0, 0));
    }

    // ---- slab staging: global (L2-resident weights) -> registers -> LDS ----
    unsigned o3[L3], o1[L1];
#pragma unroll
    for (int p = 0; p < L3; ++p) {
        const int f = tid + p * 256, row = f / KQ, kq = f % KQ;
        o3[p] = (unsigned)kq * 4u < K ? ((unsigned)row * K + (unsigned)kq * 4u) * 4u : kOut;
    }
#pragma unroll
    for (int p = 0; p < L1; ++p) {
        const int f = tid + p * 256, row = f >> 3, q4 = f & 7;
        o1[p] = row < g.C1 ? ((unsigned)row * Co + (unsigned)q4 * 4u) * 4u : kOut;
    }
    f32x4 s3[L3], s1[L1];
    auto load_slab = [&](int i) {
        const unsigned a3 = (unsigned)i * 32u * K * 4u, a1 = (unsigned)i * 128u;
#pragma unroll
        for (int p = 0; p < L3; ++p) s3[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW3, o3[p] + a3, 0, 0));
#pragma unroll
        for (int p = 0; p < L1; ++p) s1[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW1, o1[p] + a1, 0, 0));
    };
    auto store_slab = [&]() {
        float *w3s = smem, *w1s = smem + W3_SZ;
#pragma unroll
        for (int p = 0; p < L3; ++p) {
            const int f = tid + p * 256, row = f / KQ, kq = f % KQ;
            *reinterpret_cast<f32x4 *>(&w3s[row * KP + kq * 4]) = s3[p];
        }
#pragma unroll
        for (int p = 0; p < L1; ++p) {
            const int f = tid + p * 256, row = f >> 3, q4 = f & 7;
            *reinterpret_cast<f32x4 *>(&w1s[row * W1P + q4 * 4]) = s1[p];
        }
    };

    f32x16 zacc[C1T];
#pragma unroll
    for (int ct = 0; ct < C1T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) zacc[ct][r] = 0.f;

    load_slab(0);
    store_slab();
    __syncthreads();

    const int tiles = g.Co / 32;
    const float *w3s = smem, *w1s = smem + W3_SZ;
    for (int i = 0; i < tiles; ++i) {
        // residual and bias of this tile on their way under the first product (pinned: left alone, the scheduler sinks
        // them to their first use under register pressure and the epilogue waits for HBM)
        const unsigned row0 = (unsigned)(i * 32 + 4 * h);
        float rr[16];
        f32x4 bb[4];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            rr[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsR, (row0 + acc_row(r, 0)) * HW * 4u + ncol4, 0, 0));
#pragma unroll
        for (int j = 0; j < 4; ++j)
            bb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB3, (row0 + 8 * j) * 4u, 0, 0));
        __builtin_amdgcn_sched_barrier(0);

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int j = 0; j < KT * 4; ++j) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(&w3s[c * KP + 8 * j + 4 * h]);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], xr[4 * j + t], acc, 0, 0, 0);
        }
        // the Y tile: bias, residual, ReLU (the order of gemm_f32_kernel's epilogue), stored 2 rows x 128 bytes per instruction
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r];
            v += bb[r >> 2][r & 3];
            v += rr[r];
            v = __builtin_fmaxf(v, 0.f);
            acc[r] = v;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsY, (row0 + acc_row(r, 0)) * HW * 4u + ncol4, 0, 0);
        }
        // the next tile's slab (L2) on its way under the second product, into the registers the residual has left
        __builtin_amdgcn_sched_barrier(0);
        load_slab(i + 1);        // (past the last tile: offsets beyond the extent or into the next row - loaded, stored, never read)
        __builtin_amdgcn_sched_barrier(0);
        // second product: register r = 4j + t of the tile is the B operand of k = 32 i + 8j + 4h + t
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 a[C1T];
#pragma unroll
            for (int ct = 0; ct < C1T; ++ct) a[ct] = *reinterpret_cast<const f32x4 *>(&w1s[(ct * 32 + c) * W1P + 8 * j + 4 * h]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int ct = 0; ct < C1T; ++ct)
                    zacc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ct][t], acc[4 * j + t], zacc[ct], 0, 0, 0);
        }
        __syncthreads();         // every wave is done with this tile's slab
        store_slab();
        __syncthreads();
    }

    // ---- Z: bias, activation; rows beyond C1 fall past the extent ----
#pragma unroll
    for (int ct = 0; ct < C1T; ++ct) {
        const unsigned row0 = (unsigned)(ct * 32 + 4 * h);
        f32x4 bb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            bb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB1, (row0 + 8 * j) * 4u, 0, 0));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = zacc[ct][r] + bb[r >> 2][r & 3];
            if (g.relu_z) v = __builtin_fmaxf(v, 0.f);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsZ, (row0 + acc_row(r, 0)) * HW * 4u + ncol4, 0, 0);
        }
    }
}

template <int KT, int C1T>
int launch_chain(const ChainArgs &g, int batch, hipStream_t st)
{
    // measurement aid (dfx_profile_*): family -1 (the [K,N]-operand GEMM), the flops of BOTH products
    const long flops = 2L * g.HW * batch * ((long)g.Co * g.K + (long)g.C1 * g.Co);
    dfx::launch_timed(flops, -1, 32 * 1000 + 128, conv1x1_chain_kernel<KT, C1T>, dim3((unsigned)(g.nx * batch)), dim3(256), 0, st, g);
    return dfx::check_launch("conv1x1_chain_kernel");
}

}  // namespace

extern "C" int dfx_conv1x1_chain_f32(const float *W3, const float *X1, long strideX1, int K1, const float *X2, long strideX2,
                                     int K2, const float *b3, const float *R, long strideR, float *Y, long strideY,
                                     const float *W1, const float *b1, float *Z, long strideZ, int Co, int C1, int HW,
                                     int batch, int act_z, void *stream)
{
    if (Co < 0 || C1 <= 0 || HW < 0 || K1 <= 0 || K2 < 0 || batch < 0) return dfx::fail(DFX_EINVAL, "conv1x1_chain: bad dimension");
    if (act_z < 0 || act_z > 1) return dfx::fail(DFX_EINVAL, "conv1x1_chain: activation code must be 0 (none) or 1 (ReLU)");
    if ((long)Co * HW * batch == 0) return DFX_OK;
    if (!W3 || !X1 || !Y || !W1 || !Z || (K2 > 0) != (X2 != nullptr)) return dfx::fail(DFX_EINVAL, "conv1x1_chain: null pointer");
    const int K = K1 + K2;
    if ((Co & 31) || (C1 & 31) || (K1 & 15) || (K2 & 15) || (K & 31) || K > 128 || C1 > 256)
        return dfx::fail(DFX_EINVAL, "conv1x1_chain: covers Co, C1 and K multiples of 32 (segments of 16) with K <= 128, C1 <= 256");
    if ((HW & 3) || ((strideX1 | strideX2 | strideR | strideY | strideZ) & 3) || !dfx::aligned16(W3) || !dfx::aligned16(W1) ||
        !dfx::aligned16(X1) || !dfx::aligned16(Y) || !dfx::aligned16(Z) || (X2 && !dfx::aligned16(X2)) || (R && !dfx::aligned16(R)) ||
        (b3 && !dfx::aligned16(b3)) || (b1 && !dfx::aligned16(b1)))
        return dfx::fail(DFX_EINVAL, "conv1x1_chain: H*W must be a multiple of 4, buffers 16-byte aligned");
    const long nx = ((long)HW + 127) / 128;
    // 32-bit byte offsets inside one frame's operands, over the instantiated panels (up to 128 rows of X, 256 of Z)
    if ((long)(Co > 256 ? Co : 256) * HW * 4 >= (1L << 31) || (long)Co * (K > C1 ? K : C1) * 4 >= (1L << 31) || nx * batch >= (1L << 31))
        return dfx::fail(DFX_ERANGE, "conv1x1_chain: an operand exceeds 2 GiB per image");
    ChainArgs g{W3, X1, X2, b3, R, W1, b1, Y, Z, strideX1, strideX2, strideR, strideY, strideZ, K1, K, Co, C1, HW, act_z, (int)nx};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K <= 64) {
        if (C1 <= 64) return launch_chain<2, 2>(g, batch, st);
        if (C1 <= 128) return launch_chain<2, 4>(g, batch, st);
        return launch_chain<2, 8>(g, batch, st);
    }
    if (C1 <= 64) return launch_chain<4, 2>(g, batch, st);
    if (C1 <= 128) return launch_chain<4, 4>(g, batch, st);
    return launch_chain<4, 8>(g, batch, st);
}
