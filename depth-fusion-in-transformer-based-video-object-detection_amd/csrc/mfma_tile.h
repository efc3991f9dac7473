// What the fp32 MFMA kernels share (device side only, not part of the C ABI): the vector aliases, the 32 x 32 accumulator
// layout, activations, buffer descriptors and LDS-DMA; and, for the GEMM family (gemm_f32.hip, conv_igemm.hip), the geometry
// of a BM x BN workgroup tile, its K-step over the LDS stages and its epilogues - each written once.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "dfx_conv.h"

namespace dfx {
namespace mfma {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;     // (plain vectors: arrays of HIP's float4 struct can be left in scratch memory)

// row of accumulator register r in lane half h (the 32x32 MFMA accumulator layout; the column is lane & 31)
__device__ __forceinline__ constexpr int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ float activate(float v, int act)      // DFX_ACT_*: 0 passes through, exact (erf) GELU
{
    if (act == DFX_ACT_RELU) return fmaxf(v, 0.f);
    if (act == DFX_ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    return v;
}

__device__ __forceinline__ void relu4(f32x4 &v)                  // one v_max_f32 per lane (fmaxf costs a canonicalisation each)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) asm("v_max_f32 %0, 0, %1" : "=v"(v[e]) : "v"(v[e]));
}

// Buffer addressing: a wave-uniform descriptor of an operand's exact extent and a 32-bit byte offset per lane.  Whatever
// lies outside the problem gets the offset kOut, beyond every extent (operands stay below 2 GiB), and the hardware's range
// check returns zeros for its loads and drops its stores: no clamps, no selects, no 64-bit address arithmetic.
constexpr unsigned kOut = 0x80000000u;

using rsrc_t = __amdgpu_buffer_rsrc_t;
using u32x4 = __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned;
__device__ __forceinline__ rsrc_t buffer(const void *p, long bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000); }
__device__ __forceinline__ f32x4 load4(rsrc_t rs, unsigned voff, unsigned soff = 0) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0)); }
__device__ __forceinline__ float load1(rsrc_t rs, unsigned voff, unsigned soff = 0) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0)); }
__device__ __forceinline__ void store4(f32x4 v, rsrc_t rs, unsigned voff) { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, voff, 0, 0); }

// LDS-DMA (`buffer_load_dwordx4 ... lds`): 16 bytes per lane from memory straight to LDS, lane i of the wave to lds + 16 i
__device__ __forceinline__ void lds_dma16(rsrc_t rs, float *lds, unsigned voff, unsigned soff)
{
#if defined(__HIP_DEVICE_COMPILE__)      // (the host pass cannot form an LDS-address-space pointer; it only needs the kernel's handle)
    typedef __attribute__((address_space(3))) void *lds_ptr;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)lds, 16, voff, soff, 0, 0);
#else
    (void)rs; (void)lds; (void)voff; (void)soff;
#endif
}

// ---- tile geometry ------------------------------------------------------------------------------------------------------
// A workgroup of NTHR threads = WM x WN waves over a BM x BN output tile; a wave owns MT x NT MFMA tiles of 32 x 32.  The
// epilogues take the tile through LDS (row pitch LDC) in BM / PR passes of PR rows and read it back as float4: thread t
// keeps column quad t % CQ and handles NIT rows per pass, RS apart.  BAL (balanced passes): every wave writes TPP of its
// 32-row tiles per pass, where the row-range passes (BALANCE = false, or a layout that cannot balance) take tile rows
// [p PR, (p + 1) PR) and leave the waves that own none of them idle.
template <int BM_, int BN_, int WM_, int WN_, int NTHR_, bool BALANCE = true>
struct Tile {
    static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, NTHR = NTHR_;
    static constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 32, NT = TN / 32;
    static constexpr int PR = 64, LDC = BN + 4, LDB = BN + 4, CQ = BN / 4;
    static constexpr bool LEAN = NTHR % CQ == 0;                 // a thread keeps one column quad
    static constexpr int RS = LEAN ? NTHR / CQ : PR, NIT = PR / RS;
    static constexpr int TPP = PR / (32 * WM), TP1 = TPP >= 1 ? TPP : 1;
    static constexpr bool BAL = BALANCE && TPP >= 1 && PR == TPP * 32 * WM && MT % TP1 == 0;
    using RowRange = Tile<BM, BN, WM, WN, NTHR, false>;
    static_assert(NTHR == 64 * WM * WN && TM % 32 == 0 && TN % 32 == 0 && BM % PR == 0, "bad wave layout");
    static_assert(!LEAN || (PR % RS == 0 && (!BAL || (32 * TP1) % RS == 0)), "a pass is a whole number of thread rows, which do not straddle wave tiles");

    // tile row that row `row` of pass p's LDS image holds (row = it * RS for a thread's it-th float4)
    static __device__ __forceinline__ constexpr int tile_row(int p, int row)
    {
        return BAL ? (row / (32 * TP1)) * TM + p * TP1 * 32 + row % (32 * TP1) : p * PR + row;
    }
    // does MFMA tile i of the waves in wave row wm go through LDS in pass p (compile-time / wave-uniform) ...
    static __device__ __forceinline__ constexpr bool in_pass(int wm, int i, int p) { return BAL ? i / TP1 == p : (wm * TM + i * 32) / PR == p; }
    // ... and at which row of the LDS image does it start
    static __device__ __forceinline__ constexpr int lds_row(int wm, int i, int p) { return BAL ? (wm * TPP + i % TP1) * 32 : wm * TM + i * 32 - p * PR; }
};

struct Lane { int tid, wm, wn, half, c; };      // a thread's place: wave (wm, wn) of the WM x WN layout, lane half and column

template <class T>
__device__ __forceinline__ Lane lane_of(int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    return {tid, wave / T::WN, wave % T::WN, lane >> 5, lane & 31};
}

// pass p of the accumulators (a lane holds one column of 16 scattered rows) into the LDS image Ct[PR][LDC]
template <class T>
__device__ __forceinline__ void acc_to_lds(float *Ct, const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int p)
{
#pragma unroll
    for (int i = 0; i < T::MT; ++i) {
        if (!T::in_pass(l.wm, i, p)) continue;
        const int rb = T::lds_row(l.wm, i, p);
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int j = 0; j < T::NT; ++j) Ct[(rb + acc_row(r, l.half)) * T::LDC + l.wn * T::TN + j * 32 + l.c] = acc[i][j][r];
    }
}

// ---- K-steps --------------------------------------------------------------------------------------------------------------
// One stage holds BK k of the tile: As[m][k] (pitch BK + 4 floats: the 16 lanes of a ds_read_b128 group fall on 16
// different 16-byte slots) and Bs[k][n] (pitch LDB) or Bs[n][k].  The MFMA sums over k in any order as long as A and B
// agree: the BK / 2 MFMAs of a step are numbered q = 4j + t and lane (c, half) feeds MFMA q with k = 8j + 4 half + t, so one
// ds_read_b128 at [row][8j + 4 half] is the lane's operand of FOUR MFMAs.
__device__ __forceinline__ constexpr int frag_k(int q, int half) { return (q >> 2) * 8 + half * 4 + (q & 3); }

template <class T, int BK>
__device__ __forceinline__ void read_a_frags(const float *As, const Lane &l, f32x4 (&af)[BK / 8][T::MT])
{
    // (indexed as [m][k]: written as one flat index, hipcc forms an address per tile and K-step instead of one per lane + offsets)
    const float (*A)[BK + 4] = reinterpret_cast<const float (*)[BK + 4]>(As);
#pragma unroll
    for (int j = 0; j < BK / 8; ++j)
#pragma unroll
        for (int i = 0; i < T::MT; ++i) af[j][i] = *reinterpret_cast<const f32x4 *>(&A[l.wm * T::TM + i * 32 + l.c][j * 8 + l.half * 4]);
}

// MFMA group q of a K-step: b[jn] holds the lane's B value of k = frag_k(q, half)
template <class T, int BK>
__device__ __forceinline__ void mfma_group(int q, const f32x4 (&af)[BK / 8][T::MT], const float (&b)[T::NT], f32x16 (&acc)[T::MT][T::NT])
{
#pragma unroll
    for (int i = 0; i < T::MT; ++i)
#pragma unroll
        for (int jn = 0; jn < T::NT; ++jn) acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q >> 2][i][q & 3], b[jn], acc[i][jn], 0, 0, 0);
}

// [m][k] x [k][n] from register-staged LDS images (the GEMM's [K,N] operand, the implicit GEMM's gathered operand): B by
// ds_read_b32, as its rows run along n, one MFMA group ahead.
template <class T, int BK>
__device__ __forceinline__ void kstep_kn(const float *As, const float *Bs, const Lane &l, f32x16 (&acc)[T::MT][T::NT])
{
    f32x4 af[BK / 8][T::MT];
    read_a_frags<T, BK>(As, l, af);
    float bs[2][T::NT];
#pragma unroll
    for (int jn = 0; jn < T::NT; ++jn) bs[0][jn] = Bs[frag_k(0, l.half) * T::LDB + l.wn * T::TN + jn * 32 + l.c];
#pragma unroll
    for (int q = 0; q < BK / 2; ++q) {
        if (q + 1 < BK / 2) {
#pragma unroll
            for (int jn = 0; jn < T::NT; ++jn) bs[(q + 1) & 1][jn] = Bs[frag_k(q + 1, l.half) * T::LDB + l.wn * T::TN + jn * 32 + l.c];
        }
        // keep the LDS reads of the next MFMA group AHEAD of this group's MFMAs (left alone, the scheduler
        // reuses the fragment registers and sinks the reads below the MFMAs, exposing their latency)
        __builtin_amdgcn_sched_barrier(0);
        mfma_group<T, BK>(q, af, bs[q & 1], acc);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// All fragments of the K-step up front, then the MFMAs: both operands K-contiguous ([m][k] x [n][k], Linear weights: one
// ds_read_b128 per lane and 4 MFMAs each), and either form of B when the stages are filled by LDS-DMA.  hipcc orders every
// LDS read that follows an LDS-DMA in program order behind it (s_waitcnt vmcnt(0): it cannot tell the two buffers of the one
// LDS array apart), so `mid` - which issues the next tile's DMA - runs after the reads and lands under the MFMAs.
template <class T, int BK, bool B_KN, class Mid>
__device__ __forceinline__ void kstep_up_front(const float *As, const float *Bs, const Lane &l, f32x16 (&acc)[T::MT][T::NT], Mid mid)
{
    f32x4 af[BK / 8][T::MT], bf[B_KN ? 1 : BK / 8][T::NT];
    float bs[B_KN ? BK / 2 : 1][T::NT];
    read_a_frags<T, BK>(As, l, af);
#pragma unroll
    for (int q = 0; q < (B_KN ? BK / 2 : BK / 8); ++q)
#pragma unroll
        for (int jn = 0; jn < T::NT; ++jn) {
            if (B_KN) bs[B_KN ? q : 0][jn] = Bs[frag_k(q, l.half) * T::LDB + l.wn * T::TN + jn * 32 + l.c];
            else bf[B_KN ? 0 : q][jn] = *reinterpret_cast<const f32x4 *>(&Bs[(l.wn * T::TN + jn * 32 + l.c) * (BK + 4) + q * 8 + l.half * 4]);
        }
    __builtin_amdgcn_sched_barrier(0);
    mid();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < BK / 2; ++q) {
        float b[T::NT];
#pragma unroll
        for (int jn = 0; jn < T::NT; ++jn) b[jn] = B_KN ? bs[B_KN ? q : 0][jn] : bf[B_KN ? 0 : q >> 2][jn][q & 3];
        __builtin_amdgcn_sched_barrier(0);
        mfma_group<T, BK>(q, af, b, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- epilogues --------------------------------------------------------------------------------------------------------------
// C[m][n] = mask[m] ? 0 : act(acc + bias + R[m][n]) for one batch element's slices; a convolution's bias runs along the rows
struct Epilogue {
    float *C = nullptr;
    long ldc = 0;
    const float *R = nullptr;
    long ldr = 0;
    const float *bias = nullptr;
    int bias_per_row = 0;
    const unsigned char *mask = nullptr;    // per row
    int M = 0, N = 0, act = 0;
    int cblk = 0;                           // > 0: C is column-block-major, [ceil(N / cblk)][M][cblk] (scalar form only)
    long cblk_stride = 0;
};

// The lean float4 form: row-major C with 16-byte aligned rows, ReLU or no activation, C and R slices < 2 GiB.  An ablation that
// ends the tile after the K loop (profiles/r03_gemm_epilogue_ablation.txt) showed the epilogue costing 13-16 % of
// a K = 256 launch and 4-5 % of a K = 1024 one - its vector instructions take issue slots from the other resident
// workgroups' MFMAs - so it is cut to the instructions it needs:
//   every wave writes one 32-row tile per pass (was: half of the waves two tiles, the others idle);
//   a thread keeps its column quad (column bias loaded once) and its rows are m = (m0 + r0) + tile_row(pass, it RS), known
//   at compile time, so a store / residual / row-bias offset is one add to a per-thread base; C, R, the row bias and
//   the row mask go through buffer descriptors of their exact extents: rows beyond M fall past the extent (loads
//   return 0, stores are dropped), columns beyond N start from an offset beyond everything - no compares, no selects;
//   the body is compiled per (bias kind, residual, mask) instead of selecting at run time; ReLU is one v_max each.
// BIAS: 0 none, 1 per column, 2 per row.  PRE: the residual was prefetched into rpre[NIT] (the caller's 64 x 128 tile).
template <class T, int BIAS, bool HAS_R, bool HAS_MASK, bool PRE, int NPRE>
__device__ __forceinline__ void epilogue_lean(float *Ct, const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const Epilogue &e,
                                              const f32x4 (&rpre)[NPRE], bool use_rpre)
{
    static_assert(T::LEAN && (!PRE || NPRE == T::NIT), "lean epilogue: a thread keeps one column quad");
    constexpr int RS = T::RS, NIT = T::NIT;
    const int c4 = l.tid % T::CQ, r0 = l.tid / T::CQ;
    const int n = n0 + c4 * 4, mb = m0 + r0;
    const bool ncol = n < e.N;
    const unsigned cbase = ncol ? ((unsigned)mb * (unsigned)e.ldc + (unsigned)n) * 4u : kOut;
    const unsigned rbase = ncol ? ((unsigned)mb * (unsigned)e.ldr + (unsigned)n) * 4u : kOut;
    const __amdgpu_buffer_rsrc_t rsC = buffer(e.C, ((long)(e.M - 1) * e.ldc + e.N) * 4);
    const __amdgpu_buffer_rsrc_t rsR = buffer(HAS_R ? e.R : e.C, ((long)(e.M - 1) * (HAS_R ? e.ldr : e.ldc) + e.N) * 4);
    const __amdgpu_buffer_rsrc_t rsBias = buffer(BIAS ? e.bias : e.C, e.M * 4);
    const __amdgpu_buffer_rsrc_t rsMask = buffer(HAS_MASK ? (const void *)e.mask : (const void *)e.C, e.M);
    const bool relu = e.act == DFX_ACT_RELU;
    f32x4 bc = {0.f, 0.f, 0.f, 0.f};
    if (BIAS == 1 && ncol) bc = *reinterpret_cast<const f32x4 *>(e.bias + n);
    const bool r_pre = HAS_R && PRE && use_rpre;
#pragma unroll
    for (int p = 0; p < T::BM / T::PR; ++p) {
        // the residual, row bias and mask of this pass on their way while the tile goes through LDS
        f32x4 rr[HAS_R ? NIT : 1];
        float br[BIAS == 2 ? NIT : 1];
        unsigned char mk[HAS_MASK ? NIT : 1];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int D = T::tile_row(p, it * RS);
            if (HAS_R && !r_pre) rr[HAS_R ? it : 0] = load4(rsR, rbase + (unsigned)D * (unsigned)e.ldr * 4u);
            if (BIAS == 2) br[BIAS == 2 ? it : 0] = load1(rsBias, (unsigned)(mb + D) * 4u);
            if (HAS_MASK) mk[HAS_MASK ? it : 0] = __builtin_amdgcn_raw_buffer_load_b8(rsMask, (unsigned)(mb + D), 0, 0);
        }
        if (p > 0) __syncthreads();
        acc_to_lds<T>(Ct, acc, l, p);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int D = T::tile_row(p, it * RS);
            if (m0 + D >= e.M) continue;               // (scalar: the whole thread row lies beyond the last row)
            f32x4 v = *reinterpret_cast<const f32x4 *>(&Ct[(r0 + it * RS) * T::LDC + c4 * 4]);
            if (BIAS == 1) v += bc;
            if (BIAS == 2) v += br[BIAS == 2 ? it : 0];
            if (HAS_R) v += r_pre ? rpre[PRE ? it : 0] : rr[HAS_R ? it : 0];
            if (relu) relu4(v);
            if (HAS_MASK && mk[HAS_MASK ? it : 0]) v = (f32x4){0.f, 0.f, 0.f, 0.f};
            store4(v, rsC, cbase + (unsigned)D * (unsigned)e.ldc * 4u);
        }
    }
}

// ... chosen by what the launch has
template <class T, bool PRE, int NPRE>
__device__ __forceinline__ void epilogue_lean_any(float *Ct, const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const Epilogue &e,
                                                  const f32x4 (&rpre)[NPRE], bool use_rpre)
{
    auto go = [&](auto has_r, auto has_mask) {                    // compiled per (residual, mask), then per bias kind
        constexpr bool HAS_R = decltype(has_r)::value, HAS_MASK = decltype(has_mask)::value;
        if (!e.bias) epilogue_lean<T, 0, HAS_R, HAS_MASK, PRE>(Ct, acc, l, m0, n0, e, rpre, use_rpre);
        else if (e.bias_per_row) epilogue_lean<T, 2, HAS_R, HAS_MASK, PRE>(Ct, acc, l, m0, n0, e, rpre, use_rpre);
        else epilogue_lean<T, 1, HAS_R, HAS_MASK, PRE>(Ct, acc, l, m0, n0, e, rpre, use_rpre);
    };
    using Yes = std::true_type;
    using No = std::false_type;
    if (e.mask) { if (e.R) go(Yes{}, Yes{}); else go(No{}, Yes{}); }
    else { if (e.R) go(Yes{}, No{}); else go(No{}, No{}); }
}

// The general float4 form (any activation, slices of any size: pointer addressing): the accumulators go through LDS, 64 tile
// rows at a time, and leave as float4 per lane - a wave-instruction then covers whole BN*4-byte row segments (512 B for
// BN = 128) of C and of the residual instead of 128-byte pieces, with a quarter of the memory instructions.
template <class T, bool PRE, int NPRE>
__device__ __forceinline__ void epilogue_float4(float *Ct, const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const Epilogue &e,
                                                const f32x4 (&rpre)[NPRE], bool use_rpre)
{
    using G = typename T::RowRange;
    const bool brow = e.bias && e.bias_per_row, bcol = e.bias && !e.bias_per_row;
#pragma unroll
    for (int p = 0; p < T::BM / T::PR; ++p) {
        if (p > 0) __syncthreads();
        acc_to_lds<G>(Ct, acc, l, p);
        __syncthreads();
        constexpr int F4 = T::PR * T::CQ;
#pragma unroll
        for (int f0 = 0; f0 < F4; f0 += T::NTHR) {
            const int f = f0 + l.tid;
            if (F4 % T::NTHR != 0 && f >= F4) break;
            const int row = f / T::CQ, c4 = f % T::CQ;
            const int m = m0 + G::tile_row(p, row), n = n0 + c4 * 4;
            if (m >= e.M || n >= e.N) continue;
            f32x4 v = *reinterpret_cast<const f32x4 *>(&Ct[row * T::LDC + c4 * 4]);
            if (brow) v += e.bias[m];
            if (bcol) v += *reinterpret_cast<const f32x4 *>(e.bias + n);
            if (PRE && use_rpre) v += rpre[PRE ? f0 / T::NTHR : 0];
            else if (e.R) v += *reinterpret_cast<const f32x4 *>(e.R + (long)m * e.ldr + n);
            if (e.act) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = activate(v[u], e.act);
            }
            if (e.mask && e.mask[m]) v = (f32x4){0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4 *>(e.C + (long)m * e.ldc + n) = v;
        }
    }
}

// The scalar form, straight from the accumulators: N not a multiple of 4, unaligned C, column-block-major C
template <class T>
__device__ __forceinline__ void epilogue_scalar(const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const Epilogue &e)
{
    const bool brow = e.bias && e.bias_per_row, bcol = e.bias && !e.bias_per_row;
    int ncol[T::NT];
    float bcolv[T::NT];
    long coff[T::NT];                                  // element offset of the column inside a C row
    const long rowmul = e.cblk > 0 ? (long)e.cblk : e.ldc;
#pragma unroll
    for (int j = 0; j < T::NT; ++j) {
        ncol[j] = n0 + l.wn * T::TN + j * 32 + l.c;
        const int nc = min(ncol[j], e.N - 1);
        bcolv[j] = bcol ? e.bias[nc] : 0.f;
        coff[j] = e.cblk > 0 ? (long)(nc / e.cblk) * e.cblk_stride + nc % e.cblk : (long)nc;
    }
#pragma unroll
    for (int i = 0; i < T::MT; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + l.wm * T::TM + i * 32 + acc_row(r, l.half);
            const int mc = min(m, e.M - 1);                         // clamped: branch-free loads
            const float rb = brow ? e.bias[mc] : 0.f;
            const bool rz = e.mask ? e.mask[mc] != 0 : false;
#pragma unroll
            for (int j = 0; j < T::NT; ++j) {
                float v = acc[i][j][r] + bcolv[j] + rb;
                if (e.R) v += e.R[(long)mc * e.ldr + min(ncol[j], e.N - 1)];
                if (e.act) v = activate(v, e.act);
                if (rz) v = 0.f;
                if (m < e.M && ncol[j] < e.N) e.C[(long)m * rowmul + coff[j]] = v;
            }
        }
    }
}

// ---- bf16 operands (gemm_bf16.hip) -------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x16_bf16: the accumulator layout is the fp32 MFMA's (acc_row, acc_to_lds and the tile geometry above apply as
// they are); lane (c, half) holds A[row c][k = 8 half + j] and B[k = 8 half + j][col c], j = 0 .. 7, of a 16-deep step.
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// two fp32 -> one dword of two bf16 (lo in bits 0 .. 15), round-to-nearest-even: what tensor.to(torch.bfloat16) does
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi)
{
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ u32x4 pack_bf16x8(const f32x4 &a, const f32x4 &b)
{
    return (u32x4){pack_bf16(a[0], a[1]), pack_bf16(a[2], a[3]), pack_bf16(b[0], b[1]), pack_bf16(b[2], b[3])};
}

// One stage holds BK k of the tile in bf16, both operands K-contiguous: As[m][k], Bs[n][k] with a row pitch of BK + 8 elements
// (BK = 32: five 16-byte slots, so the 16 lanes of a ds_read_b128 group - 16 rows, the same k - fall on 16 different slots).
// A ds_read_b128 at [row][16 s + 8 half] is the lane's operand of the s-th 16-deep MFMA of the step.
template <class T, int BK>
__device__ __forceinline__ void kstep_bf16(const unsigned short *As, const unsigned short *Bs, const Lane &l, f32x16 (&acc)[T::MT][T::NT])
{
    constexpr int LD = BK + 8;
    bf16x8 af[BK / 16][T::MT], bf[BK / 16][T::NT];
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
#pragma unroll
        for (int i = 0; i < T::MT; ++i) af[s][i] = *reinterpret_cast<const bf16x8 *>(&As[(l.wm * T::TM + i * 32 + l.c) * LD + s * 16 + l.half * 8]);
#pragma unroll
        for (int j = 0; j < T::NT; ++j) bf[s][j] = *reinterpret_cast<const bf16x8 *>(&Bs[(l.wn * T::TN + j * 32 + l.c) * LD + s * 16 + l.half * 8]);
    }
#pragma unroll
    for (int s = 0; s < BK / 16; ++s)
#pragma unroll
        for (int i = 0; i < T::MT; ++i)
#pragma unroll
            for (int j = 0; j < T::NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
}

// C[m][n] = act(acc + bias[n] + R[m][n]) in fp32, stored as fp32 or - rounded once - as bf16
struct EpilogueOut {
    void *C = nullptr;
    long ldc = 0;
    const float *R = nullptr;
    long ldr = 0;
    const float *bias = nullptr;
    int M = 0, N = 0, act = 0;
};

// The 8-column form (N % 8 == 0, rows of C - and of R - 16-byte aligned): the tile goes through LDS as in the float4 forms, a
// thread keeps one column octet (its bias loaded once) and a row leaves as two float4 or as one 16-byte store of 8 bf16.
template <class T, bool C_BF16>
__device__ __forceinline__ void epilogue_oct(float *Ct, const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const EpilogueOut &e)
{
    constexpr int OQ = T::BN / 8, RS = T::NTHR / OQ, NIT = T::PR / RS;
    static_assert(T::NTHR % OQ == 0 && T::PR % RS == 0, "a pass is a whole number of thread rows");
    const int o = l.tid % OQ, r0 = l.tid / OQ, n = n0 + o * 8;
    const bool ncol = n < e.N;                      // (N % 8 == 0: an octet lies inside or outside)
    f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (e.bias && ncol) {
#pragma unroll
        for (int u = 0; u < 4; ++u) b0[u] = e.bias[n + u], b1[u] = e.bias[n + 4 + u];
    }
#pragma unroll
    for (int p = 0; p < T::BM / T::PR; ++p) {
        if (p > 0) __syncthreads();
        acc_to_lds<T>(Ct, acc, l, p);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = r0 + it * RS, m = m0 + T::tile_row(p, row);
            if (m >= e.M || !ncol) continue;
            f32x4 v0 = *reinterpret_cast<const f32x4 *>(&Ct[row * T::LDC + o * 8]) + b0;
            f32x4 v1 = *reinterpret_cast<const f32x4 *>(&Ct[row * T::LDC + o * 8 + 4]) + b1;
            if (e.R) {
                const f32x4 *r = reinterpret_cast<const f32x4 *>(e.R + (long)m * e.ldr + n);
                v0 += r[0], v1 += r[1];
            }
            if (e.act) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v0[u] = activate(v0[u], e.act), v1[u] = activate(v1[u], e.act);
            }
            if (C_BF16) {
                *reinterpret_cast<u32x4 *>(static_cast<unsigned short *>(e.C) + (long)m * e.ldc + n) = pack_bf16x8(v0, v1);
            } else {
                f32x4 *c = reinterpret_cast<f32x4 *>(static_cast<float *>(e.C) + (long)m * e.ldc + n);
                c[0] = v0, c[1] = v1;
            }
        }
    }
}

// The scalar form, straight from the accumulators: any N, rows of C aligned to one element only
template <class T, bool C_BF16>
__device__ __forceinline__ void epilogue_scalar_out(const f32x16 (&acc)[T::MT][T::NT], const Lane &l, int m0, int n0, const EpilogueOut &e)
{
#pragma unroll
    for (int j = 0; j < T::NT; ++j) {
        const int n = n0 + l.wn * T::TN + j * 32 + l.c;
        if (n >= e.N) continue;
        const float b = e.bias ? e.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < T::MT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + l.wm * T::TM + i * 32 + acc_row(r, l.half);
                if (m >= e.M) continue;
                float v = acc[i][j][r] + b;
                if (e.R) v += e.R[(long)m * e.ldr + n];
                if (e.act) v = activate(v, e.act);
                if (C_BF16) static_cast<unsigned short *>(e.C)[(long)m * e.ldc + n] = (unsigned short)(pack_bf16(v, v) & 0xffffu);
                else static_cast<float *>(e.C)[(long)m * e.ldc + n] = v;
            }
        }
    }
}

}  // namespace mfma
}  // namespace dfx
