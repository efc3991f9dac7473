// Weight gradient of a Linear on the bf16 matrix cores of gfx950 (include/dfx_gemm_bf16.h, dfx_gemm_bf16_wgrad):
//   dW[n][k] = sum_m bf16(dY[m][n]) bf16(X[m][k]),   db[n] = sum_m dY[m][n]   (db from the unrounded fp32 values)
// The bf16 operand path of wgrad_frame.h, which has the frame - ranges, descriptors, the double-buffered loop, the db sum, the
// reduction, the entry.  v_mfma_f32_32x32x16_bf16 wants 8 consecutive indices of the SUMMED dimension per lane, and here the
// summed dimension is the row index m of both operands - the slow one in memory.  So a step of BK = 32 rows is staged as it lies
// in memory, As[r][n] and Bs[r][k] in bf16 (two float4 -> eight bf16, round-to-nearest-even, one ds_write_b128; no bf16 copy of an
// operand reaches memory), and a lane's fragment - 8 consecutive r of ONE column - is two ds_read_b64_tr_b16, gfx950's
// transposed LDS read: per group of 16 lanes a block of 4 rows x 16 columns arrives column-major, lane 4q + p supplying the
// address of row q, columns 4p .. 4p + 3, lane i receiving column i with row q in element q.
//
// What that read needs, and how the kernel gives it:
//   EXEC all ones: the frame branches on workgroup-uniform values only, the tile is padded and nothing is masked;
//   8-byte aligned lane addresses: the row pitch is a multiple of 8 elements and a lane's column a multiple of 4;
//   no swizzle: the frame's stores and the reads here go through the one `lds_off(row, col)`, plain rows.  The pitch is BM + 32
//   (BN + 32) elements = 64 bytes beyond a multiple of 256, so the 4 rows x 64 bytes that a 32-lane half reads fall on 64
//   different banks.
#include "dfx_gemm_bf16.h"
#include "wgrad_frame.h"

namespace {

using namespace dfx::mfma;
using dfx::lds_off;

using i16x4 = __attribute__((ext_vector_type(4))) short;

// 4 consecutive rows of one column per lane (see the head of the file); `p` is the address THIS lane supplies
__device__ __forceinline__ i16x4 read_tr(const unsigned short *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) i16x4 *lds_ptr;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p);
#else
    (void)p;
    return i16x4{};
#endif
}

// rows r0 .. r0 + 7 of column (c0 + the lane's column) as one MFMA operand; `mine` = lds_off(8 half + q, 16 (group & 1) + 4 p)
template <int LD>
__device__ __forceinline__ bf16x8 frag_tr(const unsigned short *img, int mine, int s, int c0)
{
    const i16x4 lo = read_tr(img + mine + lds_off<LD>(s * 16, c0));
    const i16x4 hi = read_tr(img + mine + lds_off<LD>(s * 16 + 4, c0));
    using i16x8 = __attribute__((ext_vector_type(8))) short;
    const i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

struct WgradBf16 {
    static constexpr const char *NAME = "gemm_bf16_wgrad", *KERNEL = "gemm_bf16_wgrad_kernel";
    static constexpr int TAG = -6;                          // dfx_profile_*: flops of the product in the byte field; the reduction is -7
    static constexpr int BK = 32, G = 8, REACH = BK;        // rows per step: two 16-deep MFMAs (REACH: see the bound in wgrad_entry)
    using elem = unsigned short;
    static constexpr int pitch(int cols) { return cols + 32; }
    static __device__ __forceinline__ void put(unsigned short *dst, const f32x4 (&v)[2]) { *reinterpret_cast<u32x4 *>(dst) = pack_bf16x8(v[0], v[1]); }
    template <class T>
    struct Frags {
        static constexpr int LDA = pitch(T::BM), LDB = pitch(T::BN);
        int mineA, mineB;     // the address this lane SUPPLIES to a transposed read, relative to the block's first row and the 32-column tile's first column
        __device__ __forceinline__ explicit Frags(const Lane &l)
        {
            const int lane = l.tid & 63, gl = lane & 15, q = gl >> 2, p = gl & 3, cb = (lane >> 4 & 1) * 16;
            mineA = lds_off<LDA>(l.half * 8 + q, l.wm * T::TM + cb + 4 * p);
            mineB = lds_off<LDB>(l.half * 8 + q, l.wn * T::TN + cb + 4 * p);
        }
        __device__ __forceinline__ void kstep(const unsigned short *As, const unsigned short *Bs, const Lane &, f32x16 (&acc)[T::MT][T::NT]) const
        {
            bf16x8 af[BK / 16][T::MT], bf[BK / 16][T::NT];
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
#pragma unroll
                for (int i = 0; i < T::MT; ++i) af[s][i] = frag_tr<LDA>(As, mineA, s, i * 32);
#pragma unroll
                for (int j = 0; j < T::NT; ++j) bf[s][j] = frag_tr<LDB>(Bs, mineB, s, j * 32);
            }
#pragma unroll
            for (int s = 0; s < BK / 16; ++s)
#pragma unroll
                for (int i = 0; i < T::MT; ++i)
#pragma unroll
                    for (int j = 0; j < T::NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
        }
    };
};

}  // namespace

extern "C" int dfx_gemm_bf16_wgrad(const float *dY, long ldy, const float *X, long ldx, float *dW, long ldw, float *db,
                                   int M, int N, int K, int splits, float *workspace, void *stream)
{
    return dfx::wgrad_entry<WgradBf16>(dY, ldy, X, ldx, dW, ldw, db, M, N, K, splits, workspace, stream);
}
