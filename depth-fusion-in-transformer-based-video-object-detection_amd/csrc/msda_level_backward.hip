// grad_value of single-level fused MSDA, summed in LDS (gfx950): the value gradient of dfx_msda_fused_backward_f32 for
// the geometry of the level-in-LDS forward (msda_level.hip) without a global atomic.
//
// Geometry: L = 1, M = 8, D = 32, P = 4, fp32, a level for which dfx_msda_fused_level_fits(H, W) holds - the encoder
// self-attention, Late Fusion, Encoder Cross Fusion and the backbone fusion block of the TransVOD++ RGB-D configuration.
// msda_fused_bwd (msda_fused_backward.hip) scatters grad_value with global fp32 atomics into a zero-filled buffer, and at
// many queries that scatter is the whole cost of the backward.  Every contribution to one (frame, head, channel octet)
// slice of grad_value comes from that frame's queries, so here
//
//   workgroup = one (frame, head, channel octet) item over ALL queries of the frame (no query split: every grad_value
//               element has exactly one writer), with the forward's LDS image - bordered (H+3) x (W+2) tokens, two
//               planes of 16-byte chunks, plane stride plane_tokens(H, W) - holding ACCUMULATORS, zeroed with 16-byte
//               LDS writes at the start of each item;
//   thread    = one query at a time (1024 threads, queries strided by 1024): the forward's softmax and taps
//               (msda_level_taps.h) from the raw Linear outputs, the octet's 8 grad_out channels, then for each of the
//               16 corners corner weight x attention weight x grad_out[c] added into the 8 channels with an LDS float
//               atomic (return-less ds_add_f32);
//   flush     = after a barrier the interior H x W tokens of both planes go to grad_value[n, token, head, 8*oct ..] with
//               16-byte plain stores, zeros included: the caller allocates grad_value uninitialised.
//
// Out-of-map corners land in the zero border, which is never flushed - the trick that spares the forward its per-corner
// bounds test.  A sample that fails the in-range rule has attention weight 0 and a token index that make_taps has clamped
// into the image (y0 in [-1, H], x0 in [-1, W] for any input, NaN and infinities included), so its 16 adds of 0 go to
// border tokens: the highest float4 slot touched is PL + (H+3)*(W+2) <= 2*PL - 1.
//
// With more items than CUs the kernel is persistent like the forward (grid = CU count rounded down to a multiple of 8,
// item loop inside); the forward's item order keeps the four octets of a head, which read the same 128-byte grad_out
// rows, next to each other.
//
// Not bit-reproducible in the default mode: the order in which the LDS adds of different lanes and waves retire is not
// fixed, so two calls may differ in the last bits of grad_value - as the global-atomic route this replaces.  The three
// small gradients come from msda_fused_bwd's NEED_VALUE = false instantiation and keep their bit-reproducibility.  The
// deterministic mode runs the same kernel under its other accumulation policy (FixedSum below): sums in 64-bit fixed point.
#include "dfx_common.h"
#include "fixed_sum.h"
#include "msda_level_taps.h"

namespace {

using namespace dfx::level;

struct GradValueArgs {
    const float *ref, *off, *logits, *grad_out;
    float *grad_value;
    const void *scratch;        // FixedSum: the word enqueue_absmax leaves (fixed_sum.h); FloatSum: unused
    long off_pitch, logit_pitch;
    int H, W, Lq, PL, nitems, F;
};

// ---- the two accumulation policies ----------------------------------------------------------------------------------
// A policy owns the channels of an item (CH), the accumulator type, where token (0, 0) of the map lies in the bordered
// image, the add of one corner's CH channels, what the kernel derives once (Ctx), the 16 bytes a flush store writes and,
// on the host, what its entry checks and enqueues ahead of the launch (prepare).
// In both, token t's accumulators of a chunk start 4 * t accumulators after the origin, and out-of-map corners add into
// the border, which is never flushed.

// fp32 sums, item = channel octet: two planes of 16-byte chunks (plane c = channels 4c .. 4c+3), PL tokens apart
struct FloatSum {
    static constexpr int CH = 8;
    using Acc = float;
    struct Ctx {
        int plane;      // floats between a token's two chunks
    };
    static int prepare(const char *, const float *, long, void *, hipStream_t) { return DFX_OK; }
    static __device__ __forceinline__ Ctx context(const GradValueArgs &g) { return {4 * g.PL}; }
    static __device__ __forceinline__ Acc *origin(float4 *img, int WB) { return reinterpret_cast<Acc *>(img + WB + 1); }
    static __device__ __forceinline__ void add(Acc *d, const Ctx &c, float w, const float4 (&g)[2])
    {
        atomicAdd(d, w * g[0].x);
        atomicAdd(d + 1, w * g[0].y);
        atomicAdd(d + 2, w * g[0].z);
        atomicAdd(d + 3, w * g[0].w);
        atomicAdd(d + c.plane, w * g[1].x);
        atomicAdd(d + c.plane + 1, w * g[1].y);
        atomicAdd(d + c.plane + 2, w * g[1].z);
        atomicAdd(d + c.plane + 3, w * g[1].w);
    }
    // chunk `chunk` of bordered token `tok`
    static __device__ __forceinline__ float4 flushed(const float4 *img, const Ctx &, int PL, int tok, int chunk)
    {
        return img[chunk * PL + tok];
    }
};

// 64-bit fixed-point sums (fixed_sum.h), item = channel QUAD: 4 x int64 per token (32 bytes, token-major: the image is as
// large as FloatSum's two planes of 16 bytes, so the same levels fit).  Every add is to_fixed of FloatSum's fp32 product, so
// a sum does not depend on the order of its adds: two calls - and calls on permuted queries - give the same bits.
struct FixedSum {
    static constexpr int CH = 4;
    using Acc = unsigned long long;
    using Ctx = dfx::fixed::Scale;
    // the launch's scale: max |grad_out| into the caller's scratch word, on the stream ahead of the kernel
    static int prepare(const char *what, const float *grad_out, long n, void *scratch, hipStream_t st)
    {
        if (!scratch || !dfx::aligned16(scratch)) return dfx::fail(DFX_EINVAL, "%s: null or misaligned scratch word", what);
        return dfx::fixed::enqueue_absmax(what, grad_out, n, scratch, st);
    }
    static __device__ __forceinline__ Ctx context(const GradValueArgs &g) { return dfx::fixed::load_scale(g.scratch, g.F); }
    static __device__ __forceinline__ Acc *origin(float4 *img, int WB) { return reinterpret_cast<Acc *>(img + 2 * (WB + 1)); }
    static __device__ __forceinline__ void add(Acc *d, const Ctx &sc, float w, const float4 (&g)[1])
    {
        atomicAdd(d, dfx::fixed::to_fixed(w * g[0].x, sc.up));
        atomicAdd(d + 1, dfx::fixed::to_fixed(w * g[0].y, sc.up));
        atomicAdd(d + 2, dfx::fixed::to_fixed(w * g[0].z, sc.up));
        atomicAdd(d + 3, dfx::fixed::to_fixed(w * g[0].w, sc.up));
    }
    static __device__ __forceinline__ float4 flushed(const float4 *img, const Ctx &sc, int, int tok, int)
    {
        const longlong2 *sums = reinterpret_cast<const longlong2 *>(img);
        const longlong2 a = sums[2 * tok], b = sums[2 * tok + 1];
        return make_float4(dfx::fixed::from_fixed(a.x, sc), dfx::fixed::from_fixed(a.y, sc), dfx::fixed::from_fixed(b.x, sc),
                           dfx::fixed::from_fixed(b.y, sc));
    }
};

// item = one (frame, head, CH channels) over all queries of the frame: PARTS = 32 / CH items per (frame, head).  item & 7 is
// the head, so the parts of a (frame, head), which read the same 128-byte grad_out rows, run next to each other.
template <int REFDIM, typename SUM>
__global__ __launch_bounds__(THREADS) void msda_level_grad_value(const GradValueArgs g)
{
    constexpr int CH = SUM::CH, PARTS = 32 / CH, NQ = CH / 4;      // NQ: float4 of grad_out per query = chunks per token
    const int H = g.H, W = g.W, Lq = g.Lq, PL = g.PL;
    extern __shared__ float4 img[];                 // 2 * PL chunks of 16 bytes: the bordered image of accumulators
    const int tid = threadIdx.x;
    const int S = H * W, WB = W + 2;
    const Level lv = make_level(H, W);
    typename SUM::Acc *org = SUM::origin(img, WB);  // token (0, 0) of the map inside the bordered image
    const int row = 4 * WB;
    const typename SUM::Ctx ctx = SUM::context(g);
    // the flush's walk: NQ lanes = (token, chunk); the thread's first token and the (row, column) step between its tokens
    const int chunk = tid & (NQ - 1), tok0_y = (tid / NQ) / W, tok0_x = (tid / NQ) - tok0_y * W;
    const int step_y = (THREADS / NQ) / W, step_x = (THREADS / NQ) - step_y * W;

    // item -> (frame, head, part), the forward's order: item & 7 is the head, fixed per workgroup of the persistent grid
    for (int item = blockIdx.x; item < g.nitems; item += (int)gridDim.x) {
        const int head = item & 7, r = item >> 3;
        const int n = r / PARTS, part = r & (PARTS - 1);
        for (int j = tid; j < 2 * PL; j += THREADS) img[j] = make_float4(0.f, 0.f, 0.f, 0.f);

        const float *__restrict__ refn = g.ref + (long)n * Lq * REFDIM;
        const float *__restrict__ offn = g.off + (long)n * Lq * g.off_pitch + head * 8;
        const float *__restrict__ lgn = g.logits + (long)n * Lq * g.logit_pitch + head * 4;
        const float *__restrict__ gon = g.grad_out + (long)n * Lq * 256 + head * 32 + part * CH;
        int q = tid;
        bool have = q < Lq;
        Raw raw;
        float4 go[NQ];
        auto fetch = [&] {
            raw = load_raw<REFDIM>(refn + (long)q * REFDIM, offn + q * g.off_pitch, lgn + q * g.logit_pitch);
#pragma unroll
            for (int k = 0; k < NQ; ++k) go[k] = *reinterpret_cast<const float4 *>(gon + (long)q * 256 + 4 * k);
        };
        if (have) fetch();
        __syncthreads();                            // the image is zero before the first add

        while (have) {
            const Taps tp = make_taps<REFDIM>(raw, lv);
            float4 c[NQ];
#pragma unroll
            for (int k = 0; k < NQ; ++k) c[k] = go[k];
            // the next query's operands load under this query's adds
            q += THREADS;
            have = q < Lq;
            if (have) fetch();
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                typename SUM::Acc *d = org + 4 * tp.tb[p];
                SUM::add(d, ctx, tp.wt[p].x, c);
                SUM::add(d + 4, ctx, tp.wt[p].y, c);
                SUM::add(d + row, ctx, tp.wb[p].x, c);
                SUM::add(d + row + 4, ctx, tp.wb[p].y, c);
            }
        }
        __syncthreads();                            // every add of this item has landed

        // ---- flush the interior, zeros included: 16 bytes per (token, chunk), 4 * CH contiguous bytes per token ----
        float *__restrict__ gv = g.grad_value + (long)n * S * 256 + head * 32 + part * CH;
        // a thread's tokens are THREADS / NQ apart: (y, x) advance by (step_y, step_x) with one carry, no division per store
        for (int tok = tid / NQ, y = tok0_y, x = tok0_x; tok < S; tok += THREADS / NQ) {
            *reinterpret_cast<float4 *>(gv + (long)tok * 256 + chunk * 4) = SUM::flushed(img, ctx, PL, (y + 1) * WB + x + 1, chunk);
            x += step_x;
            y += step_y;
            if (x >= W) { x -= W; ++y; }
        }
        __syncthreads();                            // the flush has read the image before the next item zeroes it
    }
}

// the argument rules both entry points share
int check_level_args(const char *what, const float *ref, int ref_dim, const float *off, long off_pitch, const float *logits,
                     long logit_pitch, const float *grad_out, int N, int H, int W, int Lq, const float *grad_value)
{
    if (!grad_value || (Lq > 0 && (!ref || !off || !logits || !grad_out))) return dfx::fail(DFX_EINVAL, "%s: null pointer", what);
    if (ref_dim != 2 && ref_dim != 4) return dfx::fail(DFX_EINVAL, "%s: ref_dim must be 2 or 4, got %d", what, ref_dim);
    if (off_pitch < 64 || logit_pitch < 32 || ((off_pitch | logit_pitch) & 3))
        return dfx::fail(DFX_EINVAL, "%s: row pitches must be multiples of 4 floats and not smaller than "
                                     "the row (64 offsets, 32 logits)", what);
    if (!dfx::aligned16(grad_value) || !dfx::aligned16(grad_out) || !dfx::aligned16(off) || !dfx::aligned16(logits) ||
        (ref_dim == 4 ? !dfx::aligned16(ref) : ((uintptr_t)ref & 7) != 0))
        return dfx::fail(DFX_EINVAL, "%s: buffers must be 16-byte aligned", what);
    if (!dfx_msda_fused_level_fits(H, W))
        return dfx::fail(DFX_EINVAL, "%s: a %d x %d level does not fit the 160 KB LDS image; "
                                     "use the global form", what, H, W);
    if ((long)N * Lq >= (1L << 28) || (long)N * 64 >= (1L << 31)) return dfx::fail(DFX_ERANGE, "%s: too many queries or frames", what);
    return DFX_OK;
}

// Both entry points: the argument rules, the policy's own preparation, the LDS opt-in, the persistent grid, the launch.
template <typename SUM>
int launch_grad_value(const char *what, const char *kernel, const float *ref, int ref_dim, const float *off, long off_pitch,
                      const float *logits, long logit_pitch, const float *grad_out, int N, int H, int W, int Lq,
                      float *grad_value, void *scratch, void *stream)
{
    if (N < 0 || H <= 0 || W <= 0 || Lq < 0) return dfx::fail(DFX_EINVAL, "%s: bad dimension", what);
    if (N == 0) return DFX_OK;
    if (const int rc = check_level_args(what, ref, ref_dim, off, off_pitch, logits, logit_pitch, grad_out, N, H, W, Lq, grad_value))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = SUM::prepare(what, grad_out, (long)N * Lq * 256, scratch, st)) return rc;
    const int PL = (int)plane_tokens(H, W);
    const size_t lds = (size_t)2 * PL * 16;
    if (const int rc = dfx::raise_lds_limit<&msda_level_grad_value<2, SUM>, &msda_level_grad_value<4, SUM>>(what, (int)LDS_CAP))
        return rc;
    const int nitems = N * 8 * (32 / SUM::CH);
    const GradValueArgs g{ref, off, logits, grad_out, grad_value, scratch, off_pitch, logit_pitch, H, W, Lq, PL, nitems,
                          dfx::fixed::fraction_bits(dfx::fixed::msda_terms(Lq))};
    // persistent: at most one workgroup per CU, a multiple of 8 so that item & 7 (the head) is fixed per workgroup; the CU
    // count is that of the device of the first call (as the forward's grid), the machines this runs on being uniform
    static const int ncu = persistent_grid();
    const int grid = nitems < ncu ? nitems : ncu;
    const int S = H * W;
    // algorithmic bytes of this launch: grad_out + offsets + logits + reference points read, grad_value written (every
    // part of a head reads the head's offsets, logits and reference points again: not counted)
    const long bytes = 4L * ((long)N * Lq * (256 + 64 + 32 + ref_dim) + (long)N * S * 256);
    if (ref_dim == 2) dfx::launch_timed(bytes, Lq, S, msda_level_grad_value<2, SUM>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    else dfx::launch_timed(bytes, Lq, S, msda_level_grad_value<4, SUM>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    return dfx::check_launch(kernel);
}

}  // namespace

extern "C" int dfx_msda_level_grad_value_fixed_f32(const float *ref, int ref_dim, const float *off, long off_pitch,
                                                   const float *logits, long logit_pitch, const float *grad_out, int N,
                                                   int H, int W, int Lq, float *grad_value, void *scratch, void *stream)
{
    return launch_grad_value<FixedSum>("msda level grad_value (fixed)", "msda_level_grad_value_fixed", ref, ref_dim, off, off_pitch,
                                       logits, logit_pitch, grad_out, N, H, W, Lq, grad_value, scratch, stream);
}

extern "C" int dfx_msda_level_grad_value_f32(const float *ref, int ref_dim, const float *off, long off_pitch,
                                             const float *logits, long logit_pitch, const float *grad_out, int N, int H,
                                             int W, int Lq, float *grad_value, void *stream)
{
    return launch_grad_value<FloatSum>("msda level grad_value", "msda_level_grad_value", ref, ref_dim, off, off_pitch, logits,
                                       logit_pitch, grad_out, N, H, W, Lq, grad_value, nullptr, stream);
}
