// Helpers shared by the mesh kernels that take integer min / max atomics over f32 coordinates (atlas.hip's chart boxes,
// meshclean.hip's component boxes).
#pragma once
#include "common.h"

namespace lnerf {

// f32 -> u32 with the same order (negative values reversed below the positive ones, so -0 < +0)
__device__ __forceinline__ uint32_t ordered_encode(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_decode(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

}  // namespace lnerf
