// The two kernels every fixed-point gradient route shares (fixed_sum.h states the scheme): the largest |grad_out| of a
// launch as a bit pattern, and the 64-bit sums of a global workspace converted to fp32.  Both stream 16 bytes per lane.
#include "fixed_sum.h"
#include "dfx_roi.h"

namespace {

// max over x of the bit pattern of |x|: for non-negative floats the integer order is the float order, inf and NaN
// (>= 0x7f800000) above every finite number.  One integer atomic max per wave that saw a non-zero.
__global__ __launch_bounds__(256) void absmax_bits(const float4 *__restrict__ x, long n4, unsigned *__restrict__ word)
{
    unsigned m = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = x[i];
        const unsigned a = __float_as_uint(v.x) & 0x7fffffffu, b = __float_as_uint(v.y) & 0x7fffffffu;
        const unsigned c = __float_as_uint(v.z) & 0x7fffffffu, d = __float_as_uint(v.w) & 0x7fffffffu;
        m = max(m, max(max(a, b), max(c, d)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(word, m);
}

__global__ __launch_bounds__(256) void fixed_to_f32(const longlong2 *__restrict__ ws, const void *__restrict__ scratch, int F,
                                                    float4 *__restrict__ out, long n4)
{
    const dfx::fixed::Scale s = dfx::fixed::load_scale(scratch, F);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const longlong2 a = ws[2 * i], b = ws[2 * i + 1];
        out[i] = make_float4(dfx::fixed::from_fixed(a.x, s), dfx::fixed::from_fixed(a.y, s), dfx::fixed::from_fixed(b.x, s),
                             dfx::fixed::from_fixed(b.y, s));
    }
}

}  // namespace

namespace dfx {
namespace fixed {

int enqueue_absmax(const char *what, const float *x, long n, void *scratch, hipStream_t st)
{
    if (hipMemsetAsync(scratch, 0, 16, st) != hipSuccess) return fail(DFX_ELAUNCH, "%s: cannot clear the scale word", what);
    if (n <= 0) return DFX_OK;
    hipLaunchKernelGGL(absmax_bits, dim3((unsigned)grid_for(n / 4, 256, 2048)), dim3(256), 0, st,
                       reinterpret_cast<const float4 *>(x), n / 4, static_cast<unsigned *>(scratch));
    return check_launch(what);
}

int enqueue_convert(const char *what, const long long *ws, const void *scratch, int F, float *out, long n, hipStream_t st)
{
    if (n <= 0) return DFX_OK;
    hipLaunchKernelGGL(fixed_to_f32, dim3((unsigned)grid_for(n / 4, 256, 4096)), dim3(256), 0, st,
                       reinterpret_cast<const longlong2 *>(ws), scratch, F, reinterpret_cast<float4 *>(out), n / 4);
    return check_launch(what);
}

}  // namespace fixed
}  // namespace dfx

extern "C" int dfx_msda_fixed_fraction_bits(int Lq)
{
    return dfx::fixed::fraction_bits(dfx::fixed::msda_terms(Lq));
}

extern "C" int dfx_roi_align_fixed_fraction_bits(int K, int ph, int pw, int sampling_ratio)
{
    return dfx::fixed::fraction_bits(dfx::fixed::roi_terms(K, ph, pw, sampling_ratio));
}
