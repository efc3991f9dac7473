// Backward of the fused attention (include/dfx_mha.h, dfx_mha_backward_f32) on the gfx950 matrix cores, fp32
// (v_mfma_f32_32x32x2_f32): one launch, no atomics, nothing of size Lq x Lk read but the dropout mask and nothing written.
//
// The probabilities are recomputed from the saved log-sum-exp, P = exp(scale S - lse), and with delta_i = <dO_i, O_i>
//
//   dP = (dO V^T) o drop     dS = scale P o (dP - delta)     dV = (P o drop)^T dO     dQ = dS K     dK = dS^T Q
//
// dQ sums over keys, dK / dV sum over queries.  So that every gradient element is owned by ONE wave, which keeps it in its
// MFMA accumulators from the first tile to the last and stores it plainly, the grid holds workgroups of two roles (chosen by
// block index, a scalar branch), each recomputing the 32 x 32 tiles of S and dP it needs - the forward's transposed-product
// trick (csrc/mha.hip), used twice:
//
//   query role   lane = query (64 per workgroup), walks the key tiles; K and V tiles in LDS, Q and dO rows in registers
//     S^T[key][query]  = K Q^T           A = K tile,   B = Q^T (pre-scaled by scale log2 e)
//     dP^T[key][query] = V dO^T          A = V tile,   B = dO^T
//     dQ^T[d][query]  += K^T dS^T        A = K^T: K[key of register r][d = lane], B = dS^T as it stands in the accumulator layout
//   key role     lane = key (64 per workgroup), walks the query tiles; Q, dO, lse, delta of the tile in LDS, K and V rows in registers
//     S[query][key]    = Q K^T           A = Q tile,   B = K^T (pre-scaled)
//     dP[query][key]   = dO V^T          A = dO tile,  B = V^T
//     dV^T[d][key]    += dO^T (P o drop) A = dO[query of register r][d = lane], B = P o drop
//     dK^T[d][key]    += Q^T dS          A = Q[query of register r][d = lane],  B = dS
//
// A padded key (query role) or query (key role) of a partial last tile gets P = 0 exactly, and its mask value reads as 0, so it
// adds exactly zero; rows of such a tile are loaded from the last valid row, so every operand is finite.  A null grad_q
// (grad_k / grad_v) leaves the workgroups of that role out of the grid.
// LDS: two 32 x 36 tiles + lse and delta of 32 queries = 9.25 KB.  Scalar LDS reads [row][lane] are conflict-free at any pitch
// (32 consecutive banks per lane group), the ds_read_b128 of the first products at pitch 36 as in the forward.
#include "dfx_common.h"
#include "dfx_mha.h"
#include "mha_tile.h"

namespace {

using namespace dfx_mha;

// log2 e = LOG2E + LOG2E_LO to ~2^-50: 2^(s - lse log2 e) with one rounding (of the small difference), not one of lse log2 e
constexpr float LOG2E_LO = (float)(1.44269504088896340736 - (double)LOG2E);

__device__ __forceinline__ float prob(float s, float neg_lse)
{
    return __builtin_amdgcn_exp2f(fmaf(neg_lse, LOG2E_LO, fmaf(neg_lse, LOG2E, s)));
}

__device__ __forceinline__ void load16(float (&dst)[16], const float *p, float mul)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 t = *reinterpret_cast<const float4 *>(p + c * 4);
        dst[c * 4 + 0] = t.x * mul; dst[c * 4 + 1] = t.y * mul; dst[c * 4 + 2] = t.z * mul; dst[c * 4 + 3] = t.w * mul;
    }
}

__device__ __forceinline__ void store16(float *p, int half, const f32x16 &a, float mul)
{
#pragma unroll
    for (int g = 0; g < 4; ++g)                                        // registers 4g..4g+3 = channels 8g + 4*half + 0..3
        *reinterpret_cast<float4 *>(p + 8 * g + 4 * half) =
            make_float4(a[4 * g] * mul, a[4 * g + 1] * mul, a[4 * g + 2] * mul, a[4 * g + 3] * mul);
}

__global__ __launch_bounds__(64 * WAVES) void mha_bwd(const float *__restrict__ go, long go_batch, long go_row,
                                                      const float *__restrict__ q, long q_batch, long q_row,
                                                      const float *__restrict__ k, long k_batch, long k_row,
                                                      const float *__restrict__ v, long v_batch, long v_row,
                                                      const float *__restrict__ out, long o_batch, long o_row,
                                                      const float *__restrict__ lse, const float *__restrict__ drop,
                                                      float *__restrict__ gq, long gq_batch, long gq_row,
                                                      float *__restrict__ gk, long gk_batch, long gk_row,
                                                      float *__restrict__ gv, long gv_batch, long gv_row,
                                                      int query_blocks, int Lq, int Lk, float scale)
{
    __shared__ __attribute__((aligned(16))) float smem[2 * TK * KP + 2 * TK];
    float (*const as)[KP] = reinterpret_cast<float (*)[KP]>(smem);               // query role: K tile; key role: Q tile
    float (*const bs)[KP] = reinterpret_cast<float (*)[KP]>(smem + TK * KP);     // query role: V tile; key role: dO tile
    float *const lse_s = smem + 2 * TK * KP, *const del_s = lse_s + TK;          // key role: -lse and delta of the tile's queries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int hd = blockIdx.y, b = blockIdx.z;
    const long bh = (long)b * gridDim.y + hd;
    const float qs = scale * LOG2E;                                    // scores in the log2 domain, as the forward keeps them
    const bool dvec = (Lk & 3) == 0;
    q += b * q_batch + hd * D; k += b * k_batch + hd * D; v += b * v_batch + hd * D;
    go += b * go_batch + hd * D; out += b * o_batch + hd * D;

    if ((int)blockIdx.x < query_blocks) {
        // ================= query role: dQ of 64 queries =================
        const int qi = (blockIdx.x * WAVES + wave) * 32 + col, qc = min(qi, Lq - 1);
        float qv[16], dov[16];
        load16(qv, q + (long)qc * q_row + half * 16, qs);
        load16(dov, go + (long)qc * go_row + half * 16, 1.f);
        float part = 0.f;
        {
            const float *op = out + (long)qc * o_row + half * 16;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 t = *reinterpret_cast<const float4 *>(op + c * 4);
                part += dov[c * 4] * t.x + dov[c * 4 + 1] * t.y + dov[c * 4 + 2] * t.z + dov[c * 4 + 3] * t.w;
            }
        }
        const float delta = part + __shfl_xor(part, 32);
        const float nl = -lse[bh * Lq + qc];
        const float *dr = drop ? drop + (bh * Lq + qc) * Lk + 4 * half : nullptr;
        f32x16 dq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] = 0.f;
        for (int j0 = 0; j0 < Lk; j0 += TK) {
            __syncthreads();                                           // everyone is done with the previous tile
#pragma unroll
            for (int u = 0; u < (TK * D / 4) / (64 * WAVES); ++u) {
                const int e = tid + u * 64 * WAVES, r = e >> 3, c = e & 7;
                const int j = min(j0 + r, Lk - 1);
                *reinterpret_cast<float4 *>(&as[r][c * 4]) = *reinterpret_cast<const float4 *>(k + (long)j * k_row + c * 4);
                *reinterpret_cast<float4 *>(&bs[r][c * 4]) = *reinterpret_cast<const float4 *>(v + (long)j * v_row + c * 4);
            }
            __syncthreads();
            float ka[16], va[16];
            load16(ka, &as[col][half * 16], 1.f);
            load16(va, &bs[col][half * 16], 1.f);
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = 0.f;
#pragma unroll
            for (int t = 0; t < 16; ++t) s = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[t], qv[t], s, 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 16; ++t) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(va[t], dov[t], dp, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = prob(s[r], nl);
            if (j0 + TK > Lk) {                                        // (scalar: only the last tile has keys to leave out)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (j0 + acc_row(r, half) >= Lk) s[r] = 0.f;
            }
            if (dr) {                                                  // (scalar)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 d4 = drop4(dr + j0 + 8 * g, j0 + 8 * g + 4 * half, Lk, dvec);
                    dp[4 * g] *= d4.x; dp[4 * g + 1] *= d4.y; dp[4 * g + 2] *= d4.z; dp[4 * g + 3] *= d4.w;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] *= dp[r] - delta;        // dS^T / scale
#pragma unroll
            for (int r = 0; r < 16; ++r)
                dq = __builtin_amdgcn_mfma_f32_32x32x2f32(as[acc_row(r, half)][col], s[r], dq, 0, 0, 0);
        }
        if (qi < Lq) store16(gq + b * gq_batch + (long)qi * gq_row + hd * D, half, dq, scale);
        return;
    }

    // ================= key role: dK and dV of 64 keys =================
    const int kj = ((blockIdx.x - query_blocks) * WAVES + wave) * 32 + col, kc = min(kj, Lk - 1);
    float kv[16], vv[16];
    load16(kv, k + (long)kc * k_row + half * 16, qs);
    load16(vv, v + (long)kc * v_row + half * 16, 1.f);
    const float *dr = drop && kj < Lk ? drop + bh * Lq * Lk + kj : nullptr;      // (per lane) this key's mask column
    f32x16 dk, dv;
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] = 0.f, dv[r] = 0.f;
    for (int i0 = 0; i0 < Lq; i0 += TK) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < (TK * D / 4) / (64 * WAVES); ++u) {
            const int e = tid + u * 64 * WAVES, r = e >> 3, c = e & 7;
            const int i = min(i0 + r, Lq - 1);
            const float4 g4 = *reinterpret_cast<const float4 *>(go + (long)i * go_row + c * 4);
            const float4 o4 = *reinterpret_cast<const float4 *>(out + (long)i * o_row + c * 4);
            *reinterpret_cast<float4 *>(&as[r][c * 4]) = *reinterpret_cast<const float4 *>(q + (long)i * q_row + c * 4);
            *reinterpret_cast<float4 *>(&bs[r][c * 4]) = g4;
            float part = g4.x * o4.x + g4.y * o4.y + g4.z * o4.z + g4.w * o4.w;  // delta: the 8 lanes of a row, then one writes
            part += __shfl_xor(part, 1);
            part += __shfl_xor(part, 2);
            part += __shfl_xor(part, 4);
            if (c == 0) del_s[r] = part;
        }
        if (tid < TK) lse_s[tid] = -lse[bh * Lq + min(i0 + tid, Lq - 1)];
        __syncthreads();
        float qa[16], ga[16];
        load16(qa, &as[col][half * 16], 1.f);
        load16(ga, &bs[col][half * 16], 1.f);
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t], kv[t], s, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 16; ++t) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[t], vv[t], dp, 0, 0, 0);
        // register r = query i0 + acc_row(r, half): registers 4g..4g+3 are 4 consecutive queries
        float del[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 n4 = *reinterpret_cast<const float4 *>(lse_s + 8 * g + 4 * half);
            const float4 d4 = *reinterpret_cast<const float4 *>(del_s + 8 * g + 4 * half);
            s[4 * g] = prob(s[4 * g], n4.x); s[4 * g + 1] = prob(s[4 * g + 1], n4.y);
            s[4 * g + 2] = prob(s[4 * g + 2], n4.z); s[4 * g + 3] = prob(s[4 * g + 3], n4.w);
            del[4 * g] = d4.x; del[4 * g + 1] = d4.y; del[4 * g + 2] = d4.z; del[4 * g + 3] = d4.w;
        }
        if (i0 + TK > Lq) {                                            // (scalar: only the last tile has queries to leave out)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (i0 + acc_row(r, half) >= Lq) s[r] = 0.f;
        }
        f32x16 pd = s;                                                 // P o drop
        if (drop) {                                                    // (scalar)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + acc_row(r, half);
                const float m = dr && i < Lq ? dr[(long)i * Lk] : 0.f;
                pd[r] *= m;
                dp[r] *= m;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= dp[r] - del[r];           // dS / scale
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, half);
            dv = __builtin_amdgcn_mfma_f32_32x32x2f32(bs[row][col], pd[r], dv, 0, 0, 0);
            dk = __builtin_amdgcn_mfma_f32_32x32x2f32(as[row][col], s[r], dk, 0, 0, 0);
        }
    }
    if (kj < Lk) {
        store16(gk + b * gk_batch + (long)kj * gk_row + hd * D, half, dk, scale);
        store16(gv + b * gv_batch + (long)kj * gv_row + hd * D, half, dv, 1.f);
    }
}

}  // namespace

extern "C" int dfx_mha_backward_f32(const float *grad_out, long go_batch, long go_row, const float *q, long q_batch, long q_row,
                                    const float *k, long k_batch, long k_row, const float *v, long v_batch, long v_row,
                                    const float *out, long o_batch, long o_row, const float *lse, const float *drop,
                                    float *grad_q, long gq_batch, long gq_row, float *grad_k, long gk_batch, long gk_row,
                                    float *grad_v, long gv_batch, long gv_row, int B, int heads, int Lq, int Lk, float scale,
                                    void *stream)
{
    if (B < 0 || heads <= 0 || Lq < 0 || Lk < 0) return dfx::fail(DFX_EINVAL, "mha_backward: bad dimension");
    if ((grad_k == nullptr) != (grad_v == nullptr))
        return dfx::fail(DFX_EINVAL, "mha_backward: grad_k and grad_v are computed together: both or neither");
    if ((long)B * Lq == 0) return DFX_OK;
    if (Lk == 0) return dfx::fail(DFX_EINVAL, "mha_backward: no keys (softmax over an empty set)");
    if (!grad_q && !grad_k) return DFX_OK;
    if (!grad_out || !q || !k || !v || !out || !lse) return dfx::fail(DFX_EINVAL, "mha_backward: null pointer");
    if (((go_batch | go_row | q_batch | q_row | k_batch | k_row | v_batch | v_row | o_batch | o_row) & 3) ||
        (grad_q && ((gq_batch | gq_row) & 3)) || (grad_k && ((gk_batch | gk_row | gv_batch | gv_row) & 3)) ||
        !dfx::aligned16(grad_out) || !dfx::aligned16(q) || !dfx::aligned16(k) || !dfx::aligned16(v) || !dfx::aligned16(out) ||
        !dfx::aligned16(drop) || !dfx::aligned16(grad_q) || !dfx::aligned16(grad_k) || !dfx::aligned16(grad_v))
        return dfx::fail(DFX_EINVAL, "mha_backward: strides must be multiples of 4 floats, buffers 16-byte aligned");
    const int E = heads * dfx_mha::D;
    if (go_row < E || q_row < E || k_row < E || v_row < E || o_row < E || (grad_q && gq_row < E) ||
        (grad_k && (gk_row < E || gv_row < E)))
        return dfx::fail(DFX_EINVAL, "mha_backward: row strides smaller than heads * 32");
    if (B > 65535 || heads > 65535) return dfx::fail(DFX_ERANGE, "mha_backward: grid too large");
    const int per = 32 * dfx_mha::WAVES;
    const int query_blocks = grad_q ? (Lq + per - 1) / per : 0, key_blocks = grad_k ? (Lk + per - 1) / per : 0;
    const dim3 grid((unsigned)(query_blocks + key_blocks), (unsigned)heads, (unsigned)B);
    hipLaunchKernelGGL(mha_bwd, grid, dim3(64 * dfx_mha::WAVES), 0, static_cast<hipStream_t>(stream), grad_out, go_batch, go_row,
                       q, q_batch, q_row, k, k_batch, k_row, v, v_batch, v_row, out, o_batch, o_row, lse, drop, grad_q, gq_batch,
                       gq_row, grad_k, gk_batch, gk_row, grad_v, gv_batch, gv_row, query_blocks, Lq, Lk, scale);
    return dfx::check_launch("mha_bwd");
}
