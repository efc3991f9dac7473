// The reduction launch of the split weight-gradient kernels (gemm_wgrad.hip, gemm_bf16_wgrad.hip), written once: every range of
// the summed dimension left a partial [N, K] slab and, behind it, a partial db row in the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include "mfma_tile.h"

namespace dfx {
namespace {

// dW = sum_s slab_s, db = sum_s db row_s, ascending s (splits = 0: zeros); float4 per thread, the db quads follow the dW quads
__global__ void wgrad_reduce_kernel(const float *ws, int splits, long slab, long NK, int N, int K, float *dW, long ldw, float *db)
{
    using mfma::f32x4;
    const long e = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    float *dst;
    if (e < NK) {
        const long n = e / K;
        dst = dW + n * ldw + (e - n * K);
    } else if (db && e < NK + N) {
        dst = db + (e - NK);
    } else {
        return;
    }
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (splits > 0) v = *reinterpret_cast<const f32x4 *>(ws + e);
    for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const f32x4 *>(ws + (long)s * slab + e);
    dst[0] = v[0], dst[1] = v[1], dst[2] = v[2], dst[3] = v[3];
}

}  // namespace
}  // namespace dfx
