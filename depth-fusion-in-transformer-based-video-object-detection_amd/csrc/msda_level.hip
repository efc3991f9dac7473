// Fused MSDA with the whole value level resident in LDS (gfx950), for single-level attention.
//
// Geometry: L = 1, M = 8, D = 32, P = 4 - the encoder self-attention, Late Fusion, Encoder Cross
// Fusion and the backbone fusion block of the TransVOD++ RGB-D configuration (one H x W map at
// stride 16: 50 x 84 = 4200 tokens at 800 x 1333).  The wave-per-query kernel (msda_fused.hip)
// fetches every bilinear corner from L2: PMC counters show ~550 MB of L2 requests per 8-frame
// launch for 82 MB of algorithmic traffic, so it runs at the L2 gather rate (~21 TB/s), 0.39 of
// the HBM roofline.  Here the gathers are served by LDS (256 B/clk/CU, ~150 TB/s chip-wide):
//
//   workgroup = (frame, head, channel octet): 8 of the head's 32 channels of EVERY token of the
//               level - (H+3) x (W+2) x 32 B with a zero border, 146 KB of the CU's 160 KB LDS for
//               50 x 84 - staged once with 16-byte loads (each 128-byte value row is read by the
//               4 octet-workgroups of its head, which the block order puts on the same XCD/L2);
//   thread    = one query at a time (1024 threads, queries strided): softmax of the head's 4
//               logits, 4 sampling locations, then 16 corners x 2 ds_read_b128 from LDS and 128
//               FMAs into 8 accumulators; writes its 32 output bytes.
//
// LDS image: two planes of 16-byte chunks, plane c holding channels 4c..4c+3 of every bordered
// token, so the 16 lanes of a ds_read_b128 group - neighbouring queries, neighbouring tokens -
// read 16 consecutive 16-byte slots = all 64 banks once.  The zero border (one token on every
// side) stands for the out-of-map corners of the reference's bilinear rule
// (ms_deform_im2col_cuda.cuh:33-84), so a corner needs no bounds test: the sample-level skip rule
// (-1 < h < H, -1 < w < W, :281-291) zeroes the attention weight instead.  Plane stride PL is
// chosen = 4 mod 8 tokens so that a ds_write_b128 group of the staging pass (4 tokens x 2 planes)
// covers 32 distinct banks.
//
// The tap arithmetic (softmax, location, bilinear weights) is repeated by the 4 octet-workgroups
// of a head; that is the price of fitting the level into LDS, and it overlaps the staging loads of
// the first iteration.  Levels that do not fit (more than ~5100 bordered tokens) and launches
// with few queries per frame (decoder cross-attention, Lq = 300) stay on msda_fused.hip.
#include "dfx_common.h"
#include "msda_level_taps.h"
#include <stdlib.h>

namespace {

using namespace dfx::level;   // Raw, Taps, Level, make_taps, plane_tokens: msda_level_taps.h, shared with the backward

constexpr int STAGE_SLOTS = 10 * 1024;    // 2 chunks x 5120 tokens: the LDS cap (a thread stages STAGE_SLOTS / THREADS float4)

__device__ __forceinline__ void fma4(float4 &a, float w, const float4 &v)
{
    a.x = fmaf(w, v.x, a.x);
    a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z);
    a.w = fmaf(w, v.w, a.w);
}

// Operand strides (include/dfx_msda.h, dfx_msda_level_layout).  The reference layouts (value
// [N,S,8,32], one row of Linear outputs per query, out [N,Lq,256]) work, but a workgroup then uses 32
// of every 128-byte line it pulls from L2 and scatters its stores; the layouts the kernel is built for
// are the block-major ones dfx_gemm_f32 writes / reads (c_block 4 and 12, a_block), where
// everything a workgroup touches is contiguous.
struct LevelArgs {
    const float *value, *ref, *off, *logits;
    float *out;
    dfx_msda_level_layout ly;
    int H, W, Lq, PL, qsplit, nitems;
};

// Persistent: the grid is at most one workgroup per CU (146 KB of LDS each) and every workgroup walks the items
// (frame, head, octet, query slice) b, b + grid, b + 2 grid, ...: workgroup launch, index setup and the zero border are
// paid once per CU instead of once per item (4 items per CU at 32 frames).
// The schedule is stage, barrier, gather, barrier, item after item, and its phases add up (profiles/r04_level_ablate.txt).  A
// 512-thread schedule that prefetched the next item's level into registers under the gather was tried in round 4 and ran 5-8 %
// slower (profiles/r04_level_variant.txt).
template <int REFDIM>
__global__ __launch_bounds__(THREADS) void msda_fused_level(const LevelArgs g)
{
    constexpr int STAGE_PASSES = STAGE_SLOTS / THREADS;
    const int H = g.H, W = g.W, Lq = g.Lq, PL = g.PL, qsplit = g.qsplit;
    extern __shared__ float4 img[];                 // [2 planes][PL bordered tokens]
    const int tid = threadIdx.x;
    const int S = H * W, WB = W + 2;
    const int per = 4 * qsplit;
    const int qper = (Lq + qsplit - 1) / qsplit;
    Level lv;
    lv.size = (v2f){(float)W, (float)H};
    lv.rsize = (v2f){1.f / (float)W, 1.f / (float)H};
    lv.H = H; lv.W = W; lv.WB = WB;
    const long vs_token = g.ly.value_token, vs_chunk = g.ly.value_chunk;
    const long off_stride = g.ly.off_row, logit_stride = g.ly.logit_row;
    const long out_row = g.ly.out_row, out_chunk = g.ly.out_chunk;
    const int t0 = tid >> 1, c0 = tid & 1;          // staging: lane pair = (token, chunk); pass u handles token t0 + u * THREADS / 2
    const float4 *org = img + WB + 1;               // token (y, x) = (0, 0) of the map inside the bordered image

    // ---- zero border (once: staging only ever writes the interior): rows 0, H+1, H+2 and columns 0, W+1 of rows 1..H ----
    {
        const int nb = 3 * WB + 2 * H + 1;          // + the token after the last row: (y1, x1) of a sample at (H, W)
        for (int j = tid; j < 2 * nb; j += THREADS) {
            const int c = j >= nb, k = j - c * nb;
            int tb;
            if (k < WB) tb = k;
            else if (k <= 3 * WB) tb = (H + 1) * WB + (k - WB);
            else if (k <= 3 * WB + H) tb = (k - 3 * WB) * WB;
            else tb = (k - 3 * WB - H) * WB + W + 1;
            img[c * PL + tb] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // item -> (frame, head, octet, query slice).  Items go round-robin to the workgroups and the grid is a multiple of 8
    // (or the item count), so the low 3 bits - the head - are fixed per workgroup and the 4 octets (and the query
    // slices) of one (frame, head) stay on one XCD / L2.
    float4 v[STAGE_PASSES];
    // staging loads of an item: lane pair = (token, chunk), 32 contiguous bytes per token; straight-line, per-lane
    // predicated: all loads in flight at once
    auto issue_stage = [&](int item) {
        const int head = item & 7, r = item >> 3;
        const int n = r / per, oct = (r - n * per) & 3;
        const float *__restrict__ vb = g.value + n * g.ly.value_frame + head * g.ly.value_head + oct * g.ly.value_oct;
        const float *src = vb + t0 * vs_token + c0 * vs_chunk;
        const long step = (THREADS / 2) * vs_token;
#pragma unroll
        for (int u = 0; u < STAGE_PASSES; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t0 + u * (THREADS / 2) < S) v[u] = *reinterpret_cast<const float4 *>(src + u * step);
        }
    };
    // land the staged level in LDS: (y, x) of the pass's token advance by a constant step, no division
    auto land = [&]() {
        const int dy = (THREADS / 2) / W, dx = (THREADS / 2) - dy * W;
        int y = t0 / W, x = t0 - y * W;
        int idx = c0 * PL + (y + 1) * WB + x + 1;
#pragma unroll
        for (int u = 0; u < STAGE_PASSES; ++u) {
            if (t0 + u * (THREADS / 2) < S) img[idx] = v[u];
            x += dx;
            idx += dy * WB + dx;
            if (x >= W) { x -= W; idx += 2; }
        }
    };
    for (int item = blockIdx.x; item < g.nitems;) {
        const int head = item & 7, r = item >> 3;
        const int n = r / per, sub = r - n * per;
        const int oct = sub & 3, qs = sub >> 2;
        const int qbeg = qs * qper, qend = min(Lq, qbeg + qper);
        issue_stage(item);
        // ---- parameters and taps of the first query while the value loads fly ----
        const float *__restrict__ refn = g.ref + (long)n * Lq * REFDIM;
        const float *__restrict__ offn = g.off + (long)n * Lq * off_stride + head * g.ly.off_head;
        const float *__restrict__ lgn = g.logits + (long)n * Lq * logit_stride + head * g.ly.logit_head;
        float *__restrict__ outn = g.out + (long)n * Lq * g.ly.out_row + head * g.ly.out_head + oct * g.ly.out_oct;
        int q = qbeg + tid;
        bool have = q < qend;
        Raw raw;
        if (have) raw = load_raw<REFDIM>(refn + (long)q * REFDIM, offn + q * off_stride, lgn + q * logit_stride);
        Taps tp;
        if (have) tp = make_taps<REFDIM>(raw, lv);
        land();
        __syncthreads();

        // ---- gather: 16 corners x 2 chunks from LDS; the next query's parameters load meanwhile ----
        // (the grid size is read here, not at the end of the loop: with its load in the latch the compiler schedules the gather
        // with 15 registers more)
        const int next_item = item + (int)gridDim.x;
        const int iters = (qend - qbeg + THREADS - 1) / THREADS;
        for (int it = 0; it < iters; ++it) {
            const int qn = q + THREADS;
            const bool hn = qn < qend;
            if (hn) raw = load_raw<REFDIM>(refn + (long)qn * REFDIM, offn + qn * off_stride, lgn + qn * logit_stride);
            if (!have) continue;                                  // (only in a workgroup's last iteration)
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float4 *b0 = org + tp.tb[p];
                const float4 *b1 = b0 + PL;
                fma4(a0, tp.wt[p].x, b0[0]);
                fma4(a1, tp.wt[p].x, b1[0]);
                fma4(a0, tp.wt[p].y, b0[1]);
                fma4(a1, tp.wt[p].y, b1[1]);
                fma4(a0, tp.wb[p].x, b0[WB]);
                fma4(a1, tp.wb[p].x, b1[WB]);
                fma4(a0, tp.wb[p].y, b0[WB + 1]);
                fma4(a1, tp.wb[p].y, b1[WB + 1]);
            }
            float *dst = outn + q * out_row;
            *reinterpret_cast<float4 *>(dst) = a0;
            *reinterpret_cast<float4 *>(dst + out_chunk) = a1;
            if (hn) tp = make_taps<REFDIM>(raw, lv);
            q = qn;
            have = hn;
        }
        __syncthreads();                            // every gather of this item is done before the next level lands
        item = next_item;
    }
}

}  // namespace

extern "C" int dfx_msda_fused_level_fits(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return 2 * plane_tokens(H, W) * 16 <= LDS_CAP && (long)H * W * 2 <= (long)STAGE_SLOTS;
}

extern "C" int dfx_msda_fused_level_forward_f32(const float *value, const float *ref, int ref_dim, const float *off,
                                                const float *logits, const dfx_msda_level_layout *layout, int N,
                                                int H, int W, int Lq, float *out, void *stream)
{
    if (N < 0 || H <= 0 || W <= 0 || Lq < 0) return dfx::fail(DFX_EINVAL, "msda level: bad dimension");
    if (N == 0 || Lq == 0) return DFX_OK;
    if (!value || !ref || !off || !logits || !out || !layout) return dfx::fail(DFX_EINVAL, "msda level: null pointer");
    if (ref_dim != 2 && ref_dim != 4) return dfx::fail(DFX_EINVAL, "msda level: ref_dim must be 2 or 4");
    const dfx_msda_level_layout &ly = *layout;
    const long all = ly.value_frame | ly.value_token | ly.value_head | ly.value_oct | ly.value_chunk | ly.off_row |
                     ly.off_head | ly.logit_row | ly.logit_head | ly.out_row | ly.out_head | ly.out_oct | ly.out_chunk;
    if ((all & 3) || all < 0 || ly.value_token < 4 || ly.value_chunk < 4 || ly.off_row < 8 || ly.logit_row < 4 ||
        ly.out_row < 4 || ly.out_chunk < 4)
        return dfx::fail(DFX_EINVAL, "msda level: strides must be positive multiples of 4 floats (16-byte vectors)");
    if (!dfx::aligned16(value) || !dfx::aligned16(out) || !dfx::aligned16(off) || !dfx::aligned16(logits) ||
        (ref_dim == 4 ? !dfx::aligned16(ref) : ((uintptr_t)ref & 7) != 0))
        return dfx::fail(DFX_EINVAL, "msda level: buffers must be 16-byte aligned");
    if (!dfx_msda_fused_level_fits(H, W))
        return dfx::fail(DFX_EINVAL, "msda level: a %d x %d level does not fit the 160 KB LDS image; "
                                     "use dfx_msda_fused_forward_f32", H, W);
    if ((long)N * Lq >= (1L << 28)) return dfx::fail(DFX_ERANGE, "msda level: too many queries");
    // enough workgroups for the 256 CUs: split the queries of a frame when there are few frames
    int qsplit = 1;
    while ((long)N * 32 * qsplit < 256 && qsplit < 8 && Lq / (qsplit * 2) >= 512) qsplit *= 2;
    const long blocks = (long)N * 32 * qsplit;
    if (blocks >= (1L << 31)) return dfx::fail(DFX_ERANGE, "msda level: grid too large");
    const int PL = (int)plane_tokens(H, W);
    const size_t lds = (size_t)2 * PL * 16;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = dfx::raise_lds_limit<&msda_fused_level<2>, &msda_fused_level<4>>("msda level", (int)LDS_CAP)) return rc;
    const int S = H * W;
    const LevelArgs g{value, ref, off, logits, out, ly, H, W, Lq, PL, qsplit, (int)blocks};
    // persistent: at most one workgroup per CU, a multiple of 8 so that item & 7 (the head) is fixed per workgroup
    static const int ncu = persistent_grid();
    const long grid = (blocks < ncu || dfx::tuning().level_not_persistent) ? blocks : ncu;
    // algorithmic bytes of this launch: value + (offsets, logits) + out, fp32
    const long bytes = 4L * ((long)N * S * 256 + 3L * N * Lq * 8 * 4 + (long)N * Lq * 256);
    if (ref_dim == 2) dfx::launch_timed(bytes, Lq, S, msda_fused_level<2>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    else dfx::launch_timed(bytes, Lq, S, msda_fused_level<4>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    return dfx::check_launch("msda_fused_level");
}
