// Texel coordinates and bilinear taps of a texture lookup, shared by the point lookups (raster.hip) and the mip-mapped
// ones (texmip.hip), and the pyramid's packing and shape check.
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

// ---- the mip pyramid's packing, taps and shape check
// texels of levels 1 .. l - 1 of one channel in the packed buffer: sum_m (R >> m)^2 = (R^2 - (R >> (l-1))^2) / 3, exact
// because R is divisible by 2^L
__host__ __device__ __forceinline__ int64_t mip_offset(int R, int l) {
    const int64_t r0 = R, r1 = R >> (l - 1);
    return (r0 * r0 - r1 * r1) / 3;
}
static int64_t mip_texels(int R, int L) { return L > 0 ? mip_offset(R, L + 1) : 0; }

// the bilinear lookup on one level of side R: k_texture_map's mode 1 (raster.hip) and every level k_texture_mip reads
struct BilTaps {
    int64_t i00, i01, i10, i11;
    float w00, w01, w10, w11, ax, ay;   // the weights, and the fractions they are made of
};
__device__ __forceinline__ BilTaps bil_taps(float u, float v, int R) {
    float x, y;
    tex_coords(u, v, R, true, x, y);
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, R - 1), y1 = min(y0 + 1, R - 1);
    BilTaps b;
    const float ax = b.ax = x - xf, ay = b.ay = y - yf;
    b.w00 = (1.f - ax) * (1.f - ay); b.w01 = ax * (1.f - ay); b.w10 = (1.f - ax) * ay; b.w11 = ax * ay;
    b.i00 = (int64_t)y0 * R + x0; b.i01 = (int64_t)y0 * R + x1; b.i10 = (int64_t)y1 * R + x0; b.i11 = (int64_t)y1 * R + x1;
    return b;
}
__device__ __forceinline__ float bil_read(const float *tc, const BilTaps &b) {
    return b.w00 * tc[b.i00] + b.w01 * tc[b.i01] + b.w10 * tc[b.i10] + b.w11 * tc[b.i11];
}
__device__ __forceinline__ void bil_add(float *tc, const BilTaps &b, float g) {
    atomicAdd(&tc[b.i00], b.w00 * g); atomicAdd(&tc[b.i01], b.w01 * g);
    atomicAdd(&tc[b.i10], b.w10 * g); atomicAdd(&tc[b.i11], b.w11 * g);
}

// the shape of a texture and its pyramid, checked before any launch
static int check_mip_shape(const char *who, int C, int R, int L) {
    LNERF_REQUIRE(C >= 1, "%s: C must be >= 1 (got %d)", who, C);
    LNERF_REQUIRE(R >= 1, "%s: R must be >= 1 (got %d)", who, R);
    LNERF_REQUIRE(L >= 0, "%s: L must be >= 0 (got %d)", who, L);
    LNERF_REQUIRE(L <= 30 && (R & ((1 << L) - 1)) == 0, "%s: R must be divisible by 2^L (got R = %d, L = %d)", who, R, L);
    LNERF_REQUIRE((int64_t)C * R * R <= ((int64_t)1 << 38), "%s: C * R * R must be <= 2^38 (got C = %d, R = %d)", who, C, R);
    return LNERF_OK;
}

}  // namespace lnerf
