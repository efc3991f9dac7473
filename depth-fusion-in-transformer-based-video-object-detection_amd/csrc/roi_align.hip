// RoIAlign (average pooling, fixed sampling grid) for gfx950.
//
// Algorithm = mmcv 1.7.0 roi_align (avg, aligned): roi scaled by spatial_scale and shifted by
// -0.5 when aligned; each of ph x pw bins averages sampling_ratio^2 bilinear samples; a sample
// outside [-1, size] contributes 0; coordinates are clamped to [0, size-1] before interpolation.
//
// NHWC kernel: one wave per (roi, bin); lane = 4 channels, so every corner fetch of a sample is
// one fully coalesced 16-byte-per-lane read of the pixel's channel vector (1 KiB for C = 256) and
// the bin's output row leaves as one coalesced store.  The encoder memory is already token-major
// ([H*W, C]), so the reference's permute+contiguous copy to NCHW (multi_plusplus.py:498,513)
// disappears.  NCHW kernel: one thread per output element, for API parity with mmcv's layout.
//
// Backward = the transpose of that map, for the feature map only (RoIs get no gradient, as in mmcv's op):
// grad_input[b, pixel] += grad_out[k, bin] * w / sr^2 for every corner of every valid sample, by the hardware
// fp32 atomics the MSDA backward uses (unsafeAtomicAdd -> global_atomic_add_f32, no compare-and-swap loop).
// Both directions go through load_roi / locate, so they take the same skip / clamp decision for every sample.
//   roi_align_bwd_nhwc  one wave per (roi, bin) like the forward.  Lane l owns channels l, l + 64, ...: the bin's
//     grad_out row is read as coalesced 256-byte segments and every atomic wave instruction adds 256 contiguous
//     bytes of one pixel's channel row - the shape that runs at the chip-wide atomic rate.  A sample is valid when
//     ok_y & ok_x and its corner weights are (hy | ly) x (hx | lx), so the bin's whole contribution is the outer
//     product of a per-row weight vector (<= 2*sr entries) and a per-column one.  Both are built once per wave
//     (the bin is the same for all 64 lanes) with equal indices merged and zero weights dropped, which takes the
//     4*sr^2 pixel rows of the plain form (16 at sr = 2) down to 4..9 for bins narrower than two pixels.
//   roi_align_bwd_nhwc_plain  the unmerged form, four adds per sample: sampling_ratio > 4 (the merge tables hold
//     8 entries) and the A/B switch DFX_ROI_BWD_PLAIN.
//   roi_align_bwd_nchw  API parity with the NCHW forward: one thread per grad_out element, four scalar atomics per
//     sample, i.e. 64 lanes in 64 different rows per wave instruction - an order of magnitude below the shaped
//     form's atomic rate.  The model never takes it (frame_stage hands RoIAlign a channels-last view).
// Not bit-reproducible in the default mode: the arrival order of the float atomics is not fixed.  The deterministic mode
// (fixed_sum.h; dfx_roi_align_backward_nhwc_fixed_f32) instantiates the two NHWC kernels with FIXED = true: the same terms,
// added as 64-bit integers into a workspace that one more kernel converts; sampling_ratio > 0 only, the NCHW form has no twin.
#include "dfx_common.h"
#include "dfx_roi.h"
#include "fixed_sum.h"

namespace {

struct Sample {
    int yl, yh, xl, xh;
    float w1, w2, w3, w4;
    bool ok;
};

__device__ __forceinline__ Sample locate(float y, float x, int H, int W)
{
    Sample s;
    s.ok = !(y < -1.0f || y > (float)H || x < -1.0f || x > (float)W);
    if (y <= 0.f) y = 0.f;
    if (x <= 0.f) x = 0.f;
    int yl = (int)fminf(y, (float)H), xl = (int)fminf(x, (float)W);
    int yh, xh;
    if (yl >= H - 1) { yh = yl = H - 1; y = (float)yl; } else yh = yl + 1;
    if (xl >= W - 1) { xh = xl = W - 1; x = (float)xl; } else xh = xl + 1;
    const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
    s.yl = yl; s.yh = yh; s.xl = xl; s.xh = xh;
    s.w1 = hy * hx; s.w2 = hy * lx; s.w3 = ly * hx; s.w4 = ly * lx;
    return s;
}

struct Roi {
    int b;
    float x1, y1, bin_w, bin_h;
};

__device__ __forceinline__ Roi load_roi(const float *r, float scale, int aligned, int ph, int pw)
{
    Roi o;
    const float off = aligned ? 0.5f : 0.f;
    o.b = (int)r[0];
    o.x1 = r[1] * scale - off;
    o.y1 = r[2] * scale - off;
    float rw = r[3] * scale - off - o.x1, rh = r[4] * scale - off - o.y1;
    if (!aligned) { rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); }
    o.bin_w = rw / (float)pw;
    o.bin_h = rh / (float)ph;
    return o;
}

__global__ __launch_bounds__(256) void roi_align_nhwc(const float *__restrict__ in, const float *__restrict__ rois,
                                                      int N, int C, int H, int W, long nbins, int ph, int pw,
                                                      float scale, int sr, int aligned, float *__restrict__ out)
{
    const long bin = (long)blockIdx.x * 4 + (threadIdx.x >> 6);     // one wave per (roi, bin)
    if (bin >= nbins) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)(bin / (ph * pw)), ij = (int)(bin % (ph * pw));
    const int i = ij / pw, j = ij % pw;
    const Roi r = load_roi(rois + 5 * (long)k, scale, aligned, ph, pw);
    const bool live = r.b >= 0 && r.b < N;
    const float *src = in + (long)(live ? r.b : 0) * H * W * C;
    const float inv = 1.f / (float)(sr * sr);
    for (int c = lane * 4; c < C; c += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int iy = 0; iy < sr; ++iy) {
            const float y = r.y1 + i * r.bin_h + (iy + 0.5f) * r.bin_h / (float)sr;
            for (int ix = 0; ix < sr; ++ix) {
                const float x = r.x1 + j * r.bin_w + (ix + 0.5f) * r.bin_w / (float)sr;
                const Sample s = locate(y, x, H, W);
                if (!s.ok || !live) continue;
                const float4 a = *reinterpret_cast<const float4 *>(src + ((long)s.yl * W + s.xl) * C + c);
                const float4 b = *reinterpret_cast<const float4 *>(src + ((long)s.yl * W + s.xh) * C + c);
                const float4 d = *reinterpret_cast<const float4 *>(src + ((long)s.yh * W + s.xl) * C + c);
                const float4 e = *reinterpret_cast<const float4 *>(src + ((long)s.yh * W + s.xh) * C + c);
                acc.x += s.w1 * a.x + s.w2 * b.x + s.w3 * d.x + s.w4 * e.x;
                acc.y += s.w1 * a.y + s.w2 * b.y + s.w3 * d.y + s.w4 * e.y;
                acc.z += s.w1 * a.z + s.w2 * b.z + s.w3 * d.z + s.w4 * e.z;
                acc.w += s.w1 * a.w + s.w2 * b.w + s.w3 * d.w + s.w4 * e.w;
            }
        }
        acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
        *reinterpret_cast<float4 *>(out + bin * C + c) = acc;
    }
}

__global__ __launch_bounds__(256) void roi_align_nchw(const float *__restrict__ in, const float *__restrict__ rois,
                                                      int N, int C, int H, int W, long total, int ph, int pw,
                                                      float scale, int sr, int aligned, float *__restrict__ out)
{
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % pw), i = (int)((idx / pw) % ph);
        const int c = (int)((idx / ((long)pw * ph)) % C), k = (int)(idx / ((long)pw * ph * C));
        const Roi r = load_roi(rois + 5 * (long)k, scale, aligned, ph, pw);
        float acc = 0.f;
        if (r.b >= 0 && r.b < N) {
            const float *src = in + ((long)r.b * C + c) * H * W;
            for (int iy = 0; iy < sr; ++iy) {
                const float y = r.y1 + i * r.bin_h + (iy + 0.5f) * r.bin_h / (float)sr;
                for (int ix = 0; ix < sr; ++ix) {
                    const float x = r.x1 + j * r.bin_w + (ix + 0.5f) * r.bin_w / (float)sr;
                    const Sample s = locate(y, x, H, W);
                    if (!s.ok) continue;
                    acc += s.w1 * src[s.yl * W + s.xl] + s.w2 * src[s.yl * W + s.xh] +
                           s.w3 * src[s.yh * W + s.xl] + s.w4 * src[s.yh * W + s.xh];
                }
            }
        }
        out[idx] = acc / (float)(sr * sr);
    }
}

// One axis of a bin's sampling grid: (index, weight) of every map row / column some valid sample touches, equal
// indices merged, in the order met.  locate() with the other coordinate at 0 is always ok on that axis and gives
// w1 = h, w3 / w2 = l exactly (its fraction there is 0), so the decisions are the forward's, bit for bit.
template <int SR>
struct AxisTaps {
    int idx[2 * SR];
    float w[2 * SR];
    int n = 0;
    __device__ __forceinline__ void add(int at, float wgt)
    {
        if (wgt == 0.f) return;
        bool found = false;
#pragma unroll
        for (int t = 0; t < 2 * SR; ++t)
            if (t < n && idx[t] == at) { w[t] += wgt; found = true; }
        if (found) return;
#pragma unroll
        for (int t = 0; t < 2 * SR; ++t)
            if (t == n) { idx[t] = at; w[t] = wgt; }
        ++n;
    }
};

// Where the two NHWC backward kernels add (fixed_sum.h): FIXED = false is the float route, hardware fp32 atomics into
// grad_input; FIXED = true adds to_fixed(the same fp32 product) by return-less 64-bit integer atomics into an int64
// workspace laid out like grad_input, which fixed_sum.hip's convert kernel turns into grad_input.
struct FixedTarget {
    unsigned long long *ws;
    const void *scratch;
    int F;
};

template <bool FIXED>
__device__ __forceinline__ void roi_add(float *p, unsigned long long *wp, float x, double up)
{
    if constexpr (FIXED) atomicAdd(wp, dfx::fixed::to_fixed(x, up));
    else unsafeAtomicAdd(p, x);
}

template <int SR, bool FIXED = false>
__global__ __launch_bounds__(256) void roi_align_bwd_nhwc(const float *__restrict__ gout, const float *__restrict__ rois,
                                                          int N, int C, int H, int W, long nbins, int ph, int pw,
                                                          float scale, int aligned, float *__restrict__ gin, const FixedTarget fx)
{
    const long bin = (long)blockIdx.x * 4 + (threadIdx.x >> 6);     // one wave per (roi, bin)
    if (bin >= nbins) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)(bin / (ph * pw)), ij = (int)(bin % (ph * pw));
    const int i = ij / pw, j = ij % pw;
    const Roi r = load_roi(rois + 5 * (long)k, scale, aligned, ph, pw);
    if (r.b < 0 || r.b >= N) return;
    AxisTaps<SR> ty, tx;
#pragma unroll
    for (int s = 0; s < SR; ++s) {
        const float y = r.y1 + i * r.bin_h + (s + 0.5f) * r.bin_h / (float)SR;
        const Sample a = locate(y, 0.f, H, W);
        if (a.ok) { ty.add(a.yl, a.w1); ty.add(a.yh, a.w3); }
        const float x = r.x1 + j * r.bin_w + (s + 0.5f) * r.bin_w / (float)SR;
        const Sample b = locate(0.f, x, H, W);
        if (b.ok) { tx.add(b.xl, b.w1); tx.add(b.xh, b.w2); }
    }
    if (ty.n == 0 || tx.n == 0) return;
    const float inv = 1.f / (float)(SR * SR);
    float *dst = gin + (long)r.b * H * W * C;
    unsigned long long *wdst = FIXED ? fx.ws + (long)r.b * H * W * C : nullptr;
    const double up = FIXED ? dfx::fixed::load_scale(fx.scratch, fx.F).up : 0.;
    const float *g = gout + bin * C;
    for (int c = lane; c < C; c += 64) {
        const float gv = g[c] * inv;
#pragma unroll
        for (int a = 0; a < 2 * SR; ++a) {
            if (a >= ty.n) break;
#pragma unroll
            for (int b = 0; b < 2 * SR; ++b) {
                if (b >= tx.n) break;
                roi_add<FIXED>(dst + ((long)ty.idx[a] * W + tx.idx[b]) * C + c, wdst + ((long)ty.idx[a] * W + tx.idx[b]) * C + c,
                               ty.w[a] * tx.w[b] * gv, up);
            }
        }
    }
}

template <bool FIXED = false>
__global__ __launch_bounds__(256) void roi_align_bwd_nhwc_plain(const float *__restrict__ gout, const float *__restrict__ rois,
                                                                int N, int C, int H, int W, long nbins, int ph, int pw,
                                                                float scale, int sr, int aligned, float *__restrict__ gin,
                                                                const FixedTarget fx)
{
    const long bin = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bin >= nbins) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)(bin / (ph * pw)), ij = (int)(bin % (ph * pw));
    const int i = ij / pw, j = ij % pw;
    const Roi r = load_roi(rois + 5 * (long)k, scale, aligned, ph, pw);
    if (r.b < 0 || r.b >= N) return;
    const float inv = 1.f / (float)(sr * sr);
    float *dst = gin + (long)r.b * H * W * C;
    unsigned long long *wdst = FIXED ? fx.ws + (long)r.b * H * W * C : nullptr;
    const double up = FIXED ? dfx::fixed::load_scale(fx.scratch, fx.F).up : 0.;
    const float *g = gout + bin * C;
    for (int c = lane; c < C; c += 64) {
        const float gv = g[c] * inv;
        for (int iy = 0; iy < sr; ++iy) {
            const float y = r.y1 + i * r.bin_h + (iy + 0.5f) * r.bin_h / (float)sr;
            for (int ix = 0; ix < sr; ++ix) {
                const float x = r.x1 + j * r.bin_w + (ix + 0.5f) * r.bin_w / (float)sr;
                const Sample s = locate(y, x, H, W);
                if (!s.ok) continue;
                roi_add<FIXED>(dst + ((long)s.yl * W + s.xl) * C + c, wdst + ((long)s.yl * W + s.xl) * C + c, s.w1 * gv, up);
                roi_add<FIXED>(dst + ((long)s.yl * W + s.xh) * C + c, wdst + ((long)s.yl * W + s.xh) * C + c, s.w2 * gv, up);
                roi_add<FIXED>(dst + ((long)s.yh * W + s.xl) * C + c, wdst + ((long)s.yh * W + s.xl) * C + c, s.w3 * gv, up);
                roi_add<FIXED>(dst + ((long)s.yh * W + s.xh) * C + c, wdst + ((long)s.yh * W + s.xh) * C + c, s.w4 * gv, up);
            }
        }
    }
}

__global__ __launch_bounds__(256) void roi_align_bwd_nchw(const float *__restrict__ gout, const float *__restrict__ rois,
                                                          int N, int C, int H, int W, long total, int ph, int pw,
                                                          float scale, int sr, int aligned, float *__restrict__ gin)
{
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % pw), i = (int)((idx / pw) % ph);
        const int c = (int)((idx / ((long)pw * ph)) % C), k = (int)(idx / ((long)pw * ph * C));
        const Roi r = load_roi(rois + 5 * (long)k, scale, aligned, ph, pw);
        if (r.b < 0 || r.b >= N) continue;
        float *dst = gin + ((long)r.b * C + c) * H * W;
        const float gv = gout[idx] / (float)(sr * sr);
        for (int iy = 0; iy < sr; ++iy) {
            const float y = r.y1 + i * r.bin_h + (iy + 0.5f) * r.bin_h / (float)sr;
            for (int ix = 0; ix < sr; ++ix) {
                const float x = r.x1 + j * r.bin_w + (ix + 0.5f) * r.bin_w / (float)sr;
                const Sample s = locate(y, x, H, W);
                if (!s.ok) continue;
                unsafeAtomicAdd(dst + s.yl * W + s.xl, s.w1 * gv);
                unsafeAtomicAdd(dst + s.yl * W + s.xh, s.w2 * gv);
                unsafeAtomicAdd(dst + s.yh * W + s.xl, s.w3 * gv);
                unsafeAtomicAdd(dst + s.yh * W + s.xh, s.w4 * gv);
            }
        }
    }
}

int check(const void *in, const void *rois, const void *out, int N, int C, int H, int W, int K, int ph, int pw, int sr)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || K < 0 || ph <= 0 || pw <= 0)
        return dfx::fail(DFX_EINVAL, "roi_align: bad dimension");
    if (sr <= 0) return dfx::fail(DFX_EINVAL, "roi_align: sampling_ratio must be > 0 (adaptive grids are not used on this path)");
    if (K == 0) return 1;
    if (!in || !rois || !out) return dfx::fail(DFX_EINVAL, "roi_align: null pointer");
    return 0;
}

}  // namespace

extern "C" int dfx_roi_align_nhwc_f32(const float *input, const float *rois, int N, int C, int H, int W, int K,
                                      int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                      float *out, void *stream)
{
    const int rc = check(input, rois, out, N, C, H, W, K, ph, pw, sampling_ratio);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    if ((C & 3) || !dfx::aligned16(input) || !dfx::aligned16(out))
        return dfx::fail(DFX_EINVAL, "roi_align nhwc: C %% 4 == 0 and 16-byte aligned buffers required");
    const long nbins = (long)K * ph * pw;
    hipLaunchKernelGGL(roi_align_nhwc, dim3((unsigned)((nbins + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       input, rois, N, C, H, W, nbins, ph, pw, spatial_scale, sampling_ratio, aligned, out);
    return dfx::check_launch("roi_align_nhwc");
}

extern "C" int dfx_roi_align_nchw_f32(const float *input, const float *rois, int N, int C, int H, int W, int K,
                                      int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                      float *out, void *stream)
{
    const int rc = check(input, rois, out, N, C, H, W, K, ph, pw, sampling_ratio);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    const long total = (long)K * C * ph * pw;
    hipLaunchKernelGGL(roi_align_nchw, dim3(dfx::grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       input, rois, N, C, H, W, total, ph, pw, spatial_scale, sampling_ratio, aligned, out);
    return dfx::check_launch("roi_align_nchw");
}

// ---- backward: grad_input is zero-filled here, on `stream`, then accumulated into ---------------------------
namespace {

// <0: error, 1: nothing to add (grad_input zero-filled), 0: zero-filled, go on
int begin_backward(const float *grad_out, const float *rois, float *grad_input, int N, int C, int H, int W, int K,
                   int ph, int pw, int sr, bool nhwc, hipStream_t st)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || K < 0 || ph <= 0 || pw <= 0)
        return dfx::fail(DFX_EINVAL, "roi_align_backward: bad dimension");
    if (sr <= 0) return dfx::fail(DFX_EINVAL, "roi_align_backward: sampling_ratio must be > 0 (adaptive grids are not used on this path)");
    if (!grad_input || (K > 0 && (!grad_out || !rois))) return dfx::fail(DFX_EINVAL, "roi_align_backward: null pointer");
    if (nhwc && K > 0 && ((C & 3) || !dfx::aligned16(grad_out) || !dfx::aligned16(grad_input)))
        return dfx::fail(DFX_EINVAL, "roi_align_backward nhwc: C %% 4 == 0 and 16-byte aligned buffers required");
    const hipError_t e = hipMemsetAsync(grad_input, 0, (size_t)N * C * H * W * sizeof(float), st);
    if (e != hipSuccess) return dfx::fail(DFX_ELAUNCH, "roi_align_backward: zero fill: %s", hipGetErrorString(e));
    return K == 0 ? 1 : 0;
}

// the merged kernel of the sampling ratio, or the plain one (sampling_ratio > 4, DFX_ROI_BWD_PLAIN), adding by policy FIXED
template <bool FIXED>
int launch_backward_nhwc(const float *grad_out, const float *rois, int N, int C, int H, int W, int K, int ph, int pw,
                         float spatial_scale, int sampling_ratio, int aligned, float *grad_input, const FixedTarget fx,
                         hipStream_t st)
{
    const long nbins = (long)K * ph * pw;
    const dim3 grid((unsigned)((nbins + 3) / 4)), block(256);
    const int sr = dfx::tuning().roi_bwd_plain ? 0 : sampling_ratio;
#define DFX_ROI_BWD(SR)                                                                                                \
    hipLaunchKernelGGL((roi_align_bwd_nhwc<SR, FIXED>), grid, block, 0, st, grad_out, rois, N, C, H, W, nbins, ph, pw,   \
                       spatial_scale, aligned, grad_input, fx)
    switch (sr) {
    case 1: DFX_ROI_BWD(1); break;
    case 2: DFX_ROI_BWD(2); break;
    case 3: DFX_ROI_BWD(3); break;
    case 4: DFX_ROI_BWD(4); break;
    default:
        hipLaunchKernelGGL(roi_align_bwd_nhwc_plain<FIXED>, grid, block, 0, st, grad_out, rois, N, C, H, W, nbins, ph, pw,
                           spatial_scale, sampling_ratio, aligned, grad_input, fx);
    }
#undef DFX_ROI_BWD
    return dfx::check_launch("roi_align_bwd_nhwc");
}

}  // namespace

extern "C" int dfx_roi_align_backward_nhwc_f32(const float *grad_out, const float *rois, int N, int C, int H, int W, int K,
                                               int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                               float *grad_input, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = begin_backward(grad_out, rois, grad_input, N, C, H, W, K, ph, pw, sampling_ratio, true, st);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    return launch_backward_nhwc<false>(grad_out, rois, N, C, H, W, K, ph, pw, spatial_scale, sampling_ratio, aligned, grad_input,
                                       FixedTarget{}, st);
}

extern "C" int dfx_roi_align_backward_nhwc_fixed_f32(const float *grad_out, const float *rois, int N, int C, int H, int W,
                                                     int K, int ph, int pw, float spatial_scale, int sampling_ratio,
                                                     int aligned, float *grad_input, long long *workspace, void *scratch,
                                                     void *stream)
{
    const char *what = "roi_align_backward nhwc (fixed)";
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!workspace || !scratch || !dfx::aligned16(workspace) || !dfx::aligned16(scratch))
        return dfx::fail(DFX_EINVAL, "%s: null or misaligned workspace or scratch word", what);
    if (ph > 0 && pw > 0 && sampling_ratio > 0 && dfx::fixed::roi_terms(K, ph, pw, sampling_ratio) >= dfx::fixed::MAX_TERMS)
        return dfx::fail(DFX_ERANGE, "%s: too many contributions per pixel for the fixed-point sum", what);
    // the float entry's checks; its zero fill gives the K == 0 answer, and is overwritten by the convert otherwise
    const int rc = begin_backward(grad_out, rois, grad_input, N, C, H, W, K, ph, pw, sampling_ratio, true, st);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    const FixedTarget fx{reinterpret_cast<unsigned long long *>(workspace), scratch,
                         dfx::fixed::fraction_bits(dfx::fixed::roi_terms(K, ph, pw, sampling_ratio))};
    if (const int e = dfx::fixed::enqueue_absmax(what, grad_out, (long)K * ph * pw * C, scratch, st)) return e;
    if (const int e = launch_backward_nhwc<true>(grad_out, rois, N, C, H, W, K, ph, pw, spatial_scale, sampling_ratio, aligned,
                                                 grad_input, fx, st))
        return e;
    return dfx::fixed::enqueue_convert(what, workspace, scratch, fx.F, grad_input, (long)N * C * H * W, st);
}

extern "C" int dfx_roi_align_backward_nchw_f32(const float *grad_out, const float *rois, int N, int C, int H, int W, int K,
                                               int ph, int pw, float spatial_scale, int sampling_ratio, int aligned,
                                               float *grad_input, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = begin_backward(grad_out, rois, grad_input, N, C, H, W, K, ph, pw, sampling_ratio, false, st);
    if (rc < 0) return rc;
    if (rc == 1) return DFX_OK;
    const long total = (long)K * C * ph * pw;
    hipLaunchKernelGGL(roi_align_bwd_nchw, dim3(dfx::grid_for(total)), dim3(256), 0, st, grad_out, rois, N, C, H, W, total,
                       ph, pw, spatial_scale, sampling_ratio, aligned, grad_input);
    return dfx::check_launch("roi_align_bwd_nchw");
}
