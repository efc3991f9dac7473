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
// deterministic mode runs msda_level_grad_value_fixed (below) instead: the same decomposition, sums in 64-bit fixed point.
#include "dfx_common.h"
#include "fixed_sum.h"
#include "msda_level_taps.h"

namespace {

using namespace dfx::level;

struct GradValueArgs {
    const float *ref, *off, *logits, *grad_out;
    float *grad_value;
    long off_pitch, logit_pitch;
    int H, W, Lq, PL, nitems;
};

// the octet's 8 channels of one corner: token `d` of plane 0 and of plane 1 (`plane` floats further)
__device__ __forceinline__ void add_corner(float *d, int plane, float w, const float4 &g0, const float4 &g1)
{
    atomicAdd(d, w * g0.x);
    atomicAdd(d + 1, w * g0.y);
    atomicAdd(d + 2, w * g0.z);
    atomicAdd(d + 3, w * g0.w);
    atomicAdd(d + plane, w * g1.x);
    atomicAdd(d + plane + 1, w * g1.y);
    atomicAdd(d + plane + 2, w * g1.z);
    atomicAdd(d + plane + 3, w * g1.w);
}

template <int REFDIM>
__global__ __launch_bounds__(THREADS) void msda_level_grad_value(const GradValueArgs g)
{
    const int H = g.H, W = g.W, Lq = g.Lq, PL = g.PL;
    extern __shared__ float4 img[];                 // [2 planes][PL bordered tokens] of accumulators
    const int tid = threadIdx.x;
    const int S = H * W, WB = W + 2;
    const Level lv = make_level(H, W);
    float *org = reinterpret_cast<float *>(img + WB + 1);      // token (0, 0) of the map inside the bordered image
    const int plane = 4 * PL, row = 4 * WB;
    // the flush's walk: lane pair = (token, chunk); the thread's first token and the (row, column) step between its tokens
    const int chunk = tid & 1, tok0_y = (tid >> 1) / W, tok0_x = (tid >> 1) - tok0_y * W;
    const int step_y = (THREADS / 2) / W, step_x = (THREADS / 2) - step_y * W;

    // item -> (frame, head, octet), the forward's order: item & 7 is the head, fixed per workgroup of the persistent grid
    for (int item = blockIdx.x; item < g.nitems; item += (int)gridDim.x) {
        const int head = item & 7, r = item >> 3;
        const int n = r >> 2, oct = r & 3;
        for (int j = tid; j < 2 * PL; j += THREADS) img[j] = make_float4(0.f, 0.f, 0.f, 0.f);

        const float *__restrict__ refn = g.ref + (long)n * Lq * REFDIM;
        const float *__restrict__ offn = g.off + (long)n * Lq * g.off_pitch + head * 8;
        const float *__restrict__ lgn = g.logits + (long)n * Lq * g.logit_pitch + head * 4;
        const float *__restrict__ gon = g.grad_out + (long)n * Lq * 256 + head * 32 + oct * 8;
        int q = tid;
        bool have = q < Lq;
        Raw raw;
        float4 g0, g1;
        if (have) {
            raw = load_raw<REFDIM>(refn + (long)q * REFDIM, offn + q * g.off_pitch, lgn + q * g.logit_pitch);
            g0 = *reinterpret_cast<const float4 *>(gon + (long)q * 256);
            g1 = *reinterpret_cast<const float4 *>(gon + (long)q * 256 + 4);
        }
        __syncthreads();                            // the image is zero before the first add

        while (have) {
            const Taps tp = make_taps<REFDIM>(raw, lv);
            const float4 c0 = g0, c1 = g1;
            // the next query's operands load under this query's adds
            q += THREADS;
            have = q < Lq;
            if (have) {
                raw = load_raw<REFDIM>(refn + (long)q * REFDIM, offn + q * g.off_pitch, lgn + q * g.logit_pitch);
                g0 = *reinterpret_cast<const float4 *>(gon + (long)q * 256);
                g1 = *reinterpret_cast<const float4 *>(gon + (long)q * 256 + 4);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float *d = org + 4 * tp.tb[p];
                add_corner(d, plane, tp.wt[p].x, c0, c1);
                add_corner(d + 4, plane, tp.wt[p].y, c0, c1);
                add_corner(d + row, plane, tp.wb[p].x, c0, c1);
                add_corner(d + row + 4, plane, tp.wb[p].y, c0, c1);
            }
        }
        __syncthreads();                            // every add of this item has landed

        // ---- flush the interior: lane pair = (token, chunk), 32 contiguous bytes per token ----
        float *__restrict__ gv = g.grad_value + (long)n * S * 256 + head * 32 + oct * 8;
        // a thread's tokens are THREADS / 2 apart: (y, x) advance by (step_y, step_x) with one carry, no division per store
        for (int tok = tid >> 1, y = tok0_y, x = tok0_x; tok < S; tok += THREADS / 2) {
            *reinterpret_cast<float4 *>(gv + (long)tok * 256 + chunk * 4) = img[chunk * PL + (y + 1) * WB + x + 1];
            x += step_x;
            y += step_y;
            if (x >= W) { x -= W; ++y; }
        }
        __syncthreads();                            // the flush has read the image before the next item zeroes it
    }
}

// ---- the fixed-point twin (fixed_sum.h): the same decomposition with int64 accumulators ---------------------------------
// item = one (frame, head, channel QUAD) over all queries of the frame, N * 64 items; the bordered image holds 4 x int64
// per token (32 bytes, token-major: the image is as large as the float kernel's two planes of 16 bytes, so the same
// levels fit), zeroed with 16-byte LDS writes.  Every query makes 16 corners x 4 channels return-less ds_add_u64 of
// to_fixed(corner weight x attention weight x grad_out[c]), the float kernel's fp32 product.  The flush converts the
// interior to fp32 and stores 16 bytes per token: one writer per element, zeros included.  A sum does not depend on the
// order of its adds, so two calls - and calls on permuted queries - give the same bits.  Out-of-map corners add into the
// border as above; whatever gathers there is never read.  item & 7 is the head as above, so the 8 quads of a (frame, head),
// which read the same 128-byte grad_out rows, run next to each other.
struct GradValueFixedArgs {
    const float *ref, *off, *logits, *grad_out;
    float *grad_value;
    const void *scratch;
    long off_pitch, logit_pitch;
    int H, W, Lq, PL, nitems, F;
};

__device__ __forceinline__ void add_corner_fixed(unsigned long long *d, float w, const float4 &g, double up)
{
    atomicAdd(d, dfx::fixed::to_fixed(w * g.x, up));
    atomicAdd(d + 1, dfx::fixed::to_fixed(w * g.y, up));
    atomicAdd(d + 2, dfx::fixed::to_fixed(w * g.z, up));
    atomicAdd(d + 3, dfx::fixed::to_fixed(w * g.w, up));
}

template <int REFDIM>
__global__ __launch_bounds__(THREADS) void msda_level_grad_value_fixed(const GradValueFixedArgs g)
{
    const int H = g.H, W = g.W, Lq = g.Lq, PL = g.PL;
    extern __shared__ float4 img[];                 // [PL bordered tokens][4 channels] of int64 accumulators: 2 * PL chunks
    const int tid = threadIdx.x;
    const int S = H * W, WB = W + 2;
    const Level lv = make_level(H, W);
    unsigned long long *org = reinterpret_cast<unsigned long long *>(img + 2 * (WB + 1));      // token (0, 0) of the map
    const int row = 4 * WB;
    const dfx::fixed::Scale sc = dfx::fixed::load_scale(g.scratch, g.F);
    // the flush's walk: one token per thread; its first token and the (row, column) step between its tokens
    const int tok0_y = tid / W, tok0_x = tid - tok0_y * W;
    const int step_y = THREADS / W, step_x = THREADS - step_y * W;

    for (int item = blockIdx.x; item < g.nitems; item += (int)gridDim.x) {
        const int head = item & 7, r = item >> 3;
        const int n = r >> 3, quad = r & 7;
        for (int j = tid; j < 2 * PL; j += THREADS) img[j] = make_float4(0.f, 0.f, 0.f, 0.f);

        const float *__restrict__ refn = g.ref + (long)n * Lq * REFDIM;
        const float *__restrict__ offn = g.off + (long)n * Lq * g.off_pitch + head * 8;
        const float *__restrict__ lgn = g.logits + (long)n * Lq * g.logit_pitch + head * 4;
        const float *__restrict__ gon = g.grad_out + (long)n * Lq * 256 + head * 32 + quad * 4;
        int q = tid;
        bool have = q < Lq;
        Raw raw;
        float4 g0;
        if (have) {
            raw = load_raw<REFDIM>(refn + (long)q * REFDIM, offn + q * g.off_pitch, lgn + q * g.logit_pitch);
            g0 = *reinterpret_cast<const float4 *>(gon + (long)q * 256);
        }
        __syncthreads();                            // the image is zero before the first add

        while (have) {
            const Taps tp = make_taps<REFDIM>(raw, lv);
            const float4 c0 = g0;
            q += THREADS;
            have = q < Lq;
            if (have) {
                raw = load_raw<REFDIM>(refn + (long)q * REFDIM, offn + q * g.off_pitch, lgn + q * g.logit_pitch);
                g0 = *reinterpret_cast<const float4 *>(gon + (long)q * 256);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                unsigned long long *d = org + 4 * tp.tb[p];
                add_corner_fixed(d, tp.wt[p].x, c0, sc.up);
                add_corner_fixed(d + 4, tp.wt[p].y, c0, sc.up);
                add_corner_fixed(d + row, tp.wb[p].x, c0, sc.up);
                add_corner_fixed(d + row + 4, tp.wb[p].y, c0, sc.up);
            }
        }
        __syncthreads();                            // every add of this item has landed

        // ---- flush the interior: one token per thread, 4 sums -> 16 bytes of fp32 ----
        float *__restrict__ gv = g.grad_value + (long)n * S * 256 + head * 32 + quad * 4;
        const longlong2 *sums = reinterpret_cast<const longlong2 *>(img);
        for (int tok = tid, y = tok0_y, x = tok0_x; tok < S; tok += THREADS) {
            const int at = 2 * ((y + 1) * WB + x + 1);
            const longlong2 a = sums[at], b = sums[at + 1];
            *reinterpret_cast<float4 *>(gv + (long)tok * 256) =
                make_float4(dfx::fixed::from_fixed(a.x, sc), dfx::fixed::from_fixed(a.y, sc), dfx::fixed::from_fixed(b.x, sc),
                            dfx::fixed::from_fixed(b.y, sc));
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

}  // namespace

extern "C" int dfx_msda_level_grad_value_fixed_f32(const float *ref, int ref_dim, const float *off, long off_pitch,
                                                   const float *logits, long logit_pitch, const float *grad_out, int N,
                                                   int H, int W, int Lq, float *grad_value, void *scratch, void *stream)
{
    const char *what = "msda level grad_value (fixed)";
    if (N < 0 || H <= 0 || W <= 0 || Lq < 0) return dfx::fail(DFX_EINVAL, "%s: bad dimension", what);
    if (N == 0) return DFX_OK;
    if (!scratch || !dfx::aligned16(scratch)) return dfx::fail(DFX_EINVAL, "%s: null or misaligned scratch word", what);
    if (const int rc = check_level_args(what, ref, ref_dim, off, off_pitch, logits, logit_pitch, grad_out, N, H, W, Lq, grad_value))
        return rc;
    const int PL = (int)plane_tokens(H, W);
    const size_t lds = (size_t)2 * PL * 16;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = dfx::raise_lds_limit<&msda_level_grad_value_fixed<2>, &msda_level_grad_value_fixed<4>>(what, (int)LDS_CAP))
        return rc;
    if (const int rc = dfx::fixed::enqueue_absmax(what, grad_out, (long)N * Lq * 256, scratch, st)) return rc;
    const int nitems = N * 64;
    const GradValueFixedArgs g{ref, off, logits, grad_out, grad_value, scratch, off_pitch, logit_pitch, H, W, Lq, PL, nitems,
                               dfx::fixed::fraction_bits(dfx::fixed::msda_terms(Lq))};
    static const int ncu = persistent_grid();
    const int grid = nitems < ncu ? nitems : ncu;
    const int S = H * W;
    // algorithmic bytes: every quad of a head reads the head's offsets, logits and reference points again
    const long bytes = 4L * ((long)N * Lq * (256 + 64 + 32 + ref_dim) + (long)N * S * 256);
    if (ref_dim == 2) dfx::launch_timed(bytes, Lq, S, msda_level_grad_value_fixed<2>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    else dfx::launch_timed(bytes, Lq, S, msda_level_grad_value_fixed<4>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    return dfx::check_launch("msda_level_grad_value_fixed");
}

extern "C" int dfx_msda_level_grad_value_f32(const float *ref, int ref_dim, const float *off, long off_pitch,
                                             const float *logits, long logit_pitch, const float *grad_out, int N, int H,
                                             int W, int Lq, float *grad_value, void *stream)
{
    const char *what = "msda level grad_value";
    if (N < 0 || H <= 0 || W <= 0 || Lq < 0) return dfx::fail(DFX_EINVAL, "%s: bad dimension", what);
    if (N == 0) return DFX_OK;
    if (const int rc = check_level_args(what, ref, ref_dim, off, off_pitch, logits, logit_pitch, grad_out, N, H, W, Lq, grad_value))
        return rc;
    const int PL = (int)plane_tokens(H, W);
    const size_t lds = (size_t)2 * PL * 16;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = dfx::raise_lds_limit<&msda_level_grad_value<2>, &msda_level_grad_value<4>>("msda level grad_value",
                                                                                                 (int)LDS_CAP))
        return rc;
    const int nitems = N * 32;
    const GradValueArgs g{ref, off, logits, grad_out, grad_value, off_pitch, logit_pitch, H, W, Lq, PL, nitems};
    // persistent: at most one workgroup per CU, a multiple of 8 so that item & 7 (the head) is fixed per workgroup; the CU
    // count is that of the device of the first call (as the forward's grid), the machines this runs on being uniform
    static const int ncu = persistent_grid();
    const int grid = nitems < ncu ? nitems : ncu;
    const int S = H * W;
    // algorithmic bytes of this launch: grad_out + offsets + logits + reference points read, grad_value written
    const long bytes = 4L * ((long)N * Lq * (256 + 64 + 32 + ref_dim) + (long)N * S * 256);
    if (ref_dim == 2) dfx::launch_timed(bytes, Lq, S, msda_level_grad_value<2>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    else dfx::launch_timed(bytes, Lq, S, msda_level_grad_value<4>, dim3((unsigned)grid), dim3(THREADS), lds, st, g);
    return dfx::check_launch("msda_level_grad_value");
}
