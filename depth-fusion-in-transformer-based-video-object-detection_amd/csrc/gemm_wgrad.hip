// Weight gradient of a Linear on the gfx950 matrix cores (include/dfx_gemm.h, dfx_gemm_wgrad_f32): the fp32 operand path of
// wgrad_frame.h, which has the frame - ranges, descriptors, the double-buffered loop, the db sum, the reduction, the entry.
// A step of 16 rows is staged as it lies in memory, As[r][n] (pitch BM + 4) and Bs[r][k] (pitch LDB), one ds_write_b128 per
// 16-byte load, and a lane's fragment of either operand is one ds_read_b32 per MFMA - the access kstep_kn (mfma_tile.h) makes
// for its [K,N] operand, here for A as well.
#include "dfx_gemm.h"
#include "wgrad_frame.h"

namespace {

using namespace dfx::mfma;

// [k][m] x [k][n]: both fragments by ds_read_b32 (their rows run along m / n), one MFMA group ahead of the MFMAs
template <class T, int BK, int LDA>
__device__ __forceinline__ void kstep_km_kn(const float *As, const float *Bs, const Lane &l, f32x16 (&acc)[T::MT][T::NT])
{
    float a[2][T::MT], b[2][T::NT];
#pragma unroll
    for (int i = 0; i < T::MT; ++i) a[0][i] = As[frag_k(0, l.half) * LDA + l.wm * T::TM + i * 32 + l.c];
#pragma unroll
    for (int j = 0; j < T::NT; ++j) b[0][j] = Bs[frag_k(0, l.half) * T::LDB + l.wn * T::TN + j * 32 + l.c];
#pragma unroll
    for (int q = 0; q < BK / 2; ++q) {
        if (q + 1 < BK / 2) {
#pragma unroll
            for (int i = 0; i < T::MT; ++i) a[(q + 1) & 1][i] = As[frag_k(q + 1, l.half) * LDA + l.wm * T::TM + i * 32 + l.c];
#pragma unroll
            for (int j = 0; j < T::NT; ++j) b[(q + 1) & 1][j] = Bs[frag_k(q + 1, l.half) * T::LDB + l.wn * T::TN + j * 32 + l.c];
        }
        __builtin_amdgcn_sched_barrier(0);      // (as in kstep_kn: the next group's reads stay ahead of this group's MFMAs)
#pragma unroll
        for (int i = 0; i < T::MT; ++i)
#pragma unroll
            for (int j = 0; j < T::NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q & 1][i], b[q & 1][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

struct WgradF32 {
    static constexpr const char *NAME = "gemm_wgrad", *KERNEL = "gemm_wgrad_kernel";
    static constexpr int TAG = 0;                           // untimed
    static constexpr int BK = 16, G = 4, REACH = 0;         // (REACH: see the bound in wgrad_entry)
    using elem = float;
    static constexpr int pitch(int cols) { return cols + 4; }
    static __device__ __forceinline__ void put(float *dst, const f32x4 (&v)[1]) { *reinterpret_cast<f32x4 *>(dst) = v[0]; }
    template <class T>
    struct Frags {                                          // no set-up: the reads index from the lane's place itself
        __device__ __forceinline__ explicit Frags(const Lane &) {}
        __device__ __forceinline__ void kstep(const float *As, const float *Bs, const Lane &l, f32x16 (&acc)[T::MT][T::NT]) const
        {
            static_assert(pitch(T::BN) == T::LDB, "kstep_km_kn reads B at the tile's pitch");
            kstep_km_kn<T, BK, pitch(T::BM)>(As, Bs, l, acc);
        }
    };
};

}  // namespace

extern "C" int dfx_gemm_wgrad_f32(const float *dY, long ldy, const float *X, long ldx, float *dW, long ldw, float *db,
                                  int M, int N, int K, int splits, float *workspace, void *stream)
{
    return dfx::wgrad_entry<WgradF32>(dY, ldy, X, ldx, dW, ldw, db, M, N, K, splits, workspace, stream);
}
