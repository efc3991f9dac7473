// What the fused attention forward (mha.hip) and backward (mha_backward.hip) share: tile geometry and the read of the
// dropout mask by a lane that owns a QUERY (4 consecutive keys of its mask row per accumulator register group).
#pragma once
#include <hip/hip_runtime.h>
#include "mfma_tile.h"

namespace dfx_mha {

using dfx::mfma::f32x16;
using dfx::mfma::acc_row;     // row of accumulator register r in lane half h
constexpr int D = 32;          // head dimension
constexpr int TK = 32;         // rows (keys or queries) per tile
constexpr int KP = 36;         // tile row pitch (floats): 9 sixteen-byte slots, conflict-free ds_read_b128
constexpr int WAVES = 2;       // 64 queries (or keys) per workgroup
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;

// mask values of keys key0 .. key0+3 (p points at key0 of the lane's mask row); keys past Lk read as 0.
// vec: Lk % 4 == 0, so key0 (a multiple of 4) is 16-byte aligned in its row and the four keys are all in or all out.
__device__ __forceinline__ float4 drop4(const float *p, int key0, int Lk, bool vec)
{
    if (vec) return key0 < Lk ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(key0 < Lk ? p[0] : 0.f, key0 + 1 < Lk ? p[1] : 0.f, key0 + 2 < Lk ? p[2] : 0.f,
                       key0 + 3 < Lk ? p[3] : 0.f);
}

}  // namespace dfx_mha
