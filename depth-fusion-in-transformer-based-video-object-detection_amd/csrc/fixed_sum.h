// Order-independent sums for the gradients that many queries / RoIs add into (gfx950): the accumulation scheme of the
// deterministic training routes, stated once.  msda_level_backward.hip (LDS), msda_fused_backward.hip and roi_align.hip
// (global memory) include this; the two kernels they share (absmax, convert) live in fixed_sum.hip.
//
// Integer addition is associative, so a sum kept in 64-bit fixed point has the same bits for every arrival order, grid,
// wave schedule and query order.  gfx950 adds 64-bit integers without a return value in LDS (ds_add_u64) and in global
// memory (global_atomic_add_x2); neither is a compare-and-swap loop.
//
// Scale.   gmax = max |grad_out| over the launch, found on the device (enqueue_absmax: wave maxima of the bit pattern
//          of |x| joined by an integer atomic max - a max does not depend on order either) and left in the first word
//          of a caller-owned 16-byte scratch; the host never reads it.  e = the exponent with gmax < 2^e
//          (biased exponent field - 126; a denormal gmax takes -125).
// Bound.   n = a HOST upper bound on the number of contributions that can meet in one accumulator:
//            MSDA      one accumulator is a channel of one token of one (frame, head, level).  What can reach it are the
//                      (query, point, corner) triples of that frame's queries at that head and level: n = Lq * P * 4 =
//                      16 * Lq.  (The four corners of one point are four different tokens, so Lq * P would do; counting
//                      the triples costs two fraction bits and needs no argument about clamped or merged corners.)
//            RoIAlign  one accumulator is a channel of one pixel.  Every (RoI, bin, sample, corner) can add there once:
//                      n = 4 * sr^2 * ph * pw * K.  The merged form adds fewer, larger terms (one per (row, column)
//                      pair of a bin), each the sum of the plain form's terms it replaces.
//          F = min(50, 61 - ceil(log2 n)) fraction bits below 2^e.
// Term.    Every contribution c is computed in fp32 exactly as the float route computes it - (weights <= 1) x grad_out,
//          so |c| <= gmax < 2^e up to the rounding of the weights' product - then scaled by the power of two 2^(F-e)
//          (exact in fp64) and rounded to the nearest integer: |c * 2^(F-e)| < 2^F <= 2^50, inside the range 2^51 of
//          the add-and-subtract-1.5*2^52 rounding of to_fixed.  n terms sum to less than n * 2^F <= 2^61: two bits
//          below the wrap of a signed 64-bit sum, which is the room for weights a few ulp above 1.
// Adds.    Return-less 64-bit integer atomics on the two's complement pattern.
// Result.  sum * 2^(e-F) rounded to fp32 by one fixed sequence (from_fixed: int64 -> fp64, one exact power-of-two
//          product, fp64 -> fp32).  Scaling grad_out by a power of two scales the result by it exactly.
// Edges.   gmax == 0, no queries, no RoIs: every term and every sum is the integer 0, every element an exact +0.
//          A NON-FINITE gmax (any inf or NaN in grad_out: as a bit pattern both are >= 0x7f800000, so the integer max
//          keeps them) makes EVERY element of that launch's gradient NaN - deterministic and loud; the float routes
//          would have put inf / NaN into the elements those rows reach only.
#pragma once
#include "dfx_common.h"

namespace dfx {
namespace fixed {

constexpr int MAX_FRACTION_BITS = 50;
constexpr long MAX_TERMS = 1L << 32;        // F >= 29 below it: an entry point refuses a launch whose bound is larger

// F of the header: n >= 1 terms of magnitude below 2^F sum to less than 2^61
inline int fraction_bits(long n)
{
    int lg = 0;
    while (lg < 62 && (1L << lg) < n) ++lg;     // ceil(log2 n)
    const int f = 61 - lg;
    return f < MAX_FRACTION_BITS ? f : MAX_FRACTION_BITS;
}

inline long msda_terms(int Lq) { return 16L * (Lq > 0 ? Lq : 1); }
inline long roi_terms(int K, int ph, int pw, int sr)      // saturates at 2^62 (far above MAX_TERMS) instead of wrapping
{
    const double n = 4.0 * sr * sr * ph * pw * (K > 0 ? K : 1);
    return n < 0x1p62 ? (long)n : 1L << 62;
}

// zero the scratch word and leave the bit pattern of max |x[0 .. n)| in it (n a multiple of 4, x 16-byte aligned);
// n == 0 leaves 0.  Enqueue-only.
int enqueue_absmax(const char *what, const float *x, long n, void *scratch, hipStream_t st);
// out[i] = ws[i] * 2^(e-F) for i in [0, n), n a multiple of 4, both 16-byte aligned (NaN everywhere for a non-finite gmax)
int enqueue_convert(const char *what, const long long *ws, const void *scratch, int F, float *out, long n, hipStream_t st);

#ifdef __HIPCC__
// What a kernel derives from the scratch word: 2^(F-e), 2^(e-F) and whether gmax is finite.
struct Scale {
    double up, down;
    bool finite;
};

__device__ __forceinline__ Scale load_scale(const void *scratch, int F)
{
    const unsigned bits = *static_cast<const unsigned *>(scratch);
    const int field = (int)(bits >> 23);                // biased exponent of gmax: gmax < 2^(field - 126)
    const int e = (field ? field : 1) - 126;
    Scale s;
    s.up = __longlong_as_double((long long)(1023 + F - e) << 52);
    s.down = __longlong_as_double((long long)(1023 + e - F) << 52);
    s.finite = field != 255;
    return s;
}

// rint(c * 2^(F-e)) as a two's complement pattern: the product is exact in fp64, adding 1.5 * 2^52 leaves the rounded
// integer in the low mantissa bits for |product| < 2^51, and the 64-bit subtract takes the constant's pattern away
__device__ __forceinline__ unsigned long long to_fixed(float c, double up)
{
    const double d = __builtin_fma((double)c, up, 0x1.8p52);
    return (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000LL);
}

__device__ __forceinline__ float from_fixed(long long sum, const Scale &s)
{
    return s.finite ? (float)((double)sum * s.down) : __builtin_nanf("");
}
#endif

}  // namespace fixed
}  // namespace dfx
