// Texel coordinates of a texture lookup, shared by the point lookups (raster.hip) and the mip-mapped one (texmip.hip).
#pragma once
#include "common.h"

namespace lnerf {

// texture lookup: tex [C,R,R]; uv [P,2]; grid_sample(align_corners=False, border) on (u, 1 - v) after clamping uv to
// [0, 1] (the semantics of kal.render.mesh.texture_mapping, the op the reference calls at
// src/latent_paint/models/render.py:64 with mode = guide.texture_interpolation_mode)
__device__ __forceinline__ void tex_coords(float u, float v, int R, bool clip, float &x, float &y) {
    u = clampf(u, 0.f, 1.f);
    v = clampf(v, 0.f, 1.f);
    const float gx = u * 2.0f - 1.0f, gy = -(v * 2.0f - 1.0f);
    x = ((gx + 1.0f) * (float)R - 1.0f) * 0.5f;
    y = ((gy + 1.0f) * (float)R - 1.0f) * 0.5f;
    if (clip) {  // padding_mode = 'border' (nearest / bilinear clip the position, bicubic clips every tap instead)
        x = clampf(x, 0.f, (float)(R - 1));
        y = clampf(y, 0.f, (float)(R - 1));
    }
}

}  // namespace lnerf
