// Which views a surface point accepts, and the bilinear sample it takes there: steps 1-5 of the projection rule
// (include/lnerf_hip.h, lnerf_uv_project_views) and the nested lerps of step 6, shared by the plain projection
// (uvproject.hip) and the exposure / two-band kernels (viewblend.hip), so that all of them take the same decisions.
#pragma once
#include "common.h"
#include "raster_shared.h"

namespace lnerf {

constexpr int PROJ_THREADS = 256;
constexpr int PROJ_CAM_TILE = 64;   // camera records per LDS tile (64 * CAM_FLOATS floats = 3.5 KiB)
constexpr int PROJ_MAX_C = 4;

// an accepted (point, view) pair: the cosine of step 1, the top-left tap's offset i0 * W + j0 in a [H,W] plane and the
// fractions of step 3
struct ViewTap {
    float c, tu, tv;
    int64_t off;
};

// steps 1-5 for the point x (unit normal n) and the view with record `cam` and depth plane `zplane` [H,W]
__device__ __forceinline__ bool view_accept(const float *x, const float *n, const float *cam, const float *zplane, int W,
                                            float Wf, float Hf, float cos_min, float slack, ViewTap &t) {
    // 1. the angle between the normal and the direction to the eye
    const float dx = cam[CAM_POS] - x[0], dy = cam[CAM_POS + 1] - x[1], dz = cam[CAM_POS + 2] - x[2];
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    const float c = (n[0] * dx + n[1] * dy + n[2] * dz) / len;
    if (!(c >= cos_min)) return false;
    // 2. camera space: the rasteriser's own projection (raster_shared.h)
    const auto [pz, X, Y] = cam_project(cam, x[0], x[1], x[2]);
    if (!(pz < 0.f)) return false;
    const float fx = cam[CAM_FX], fy = cam[CAM_FY];
    // 3. pixel coordinates, pixel centres at integers; all four taps inside the image
    const float u = ndc_to_col(X, Wf), v = ndc_to_row(Y, Hf);
    if (!(u >= 0.f && u < Wf - 1.0f && v >= 0.f && v < Hf - 1.0f)) return false;
    const float uf = floorf(u), vf = floorf(v);
    const int j0 = (int)uf, i0 = (int)vf;
    const float tu = u - uf, tv = v - vf;
    // 4. no tap on the background or on an eroded pixel
    const int64_t off = (int64_t)i0 * W + j0;
    const float *zb = zplane + off;
    const float z00 = zb[0], z01 = zb[1], z10 = zb[W], z11 = zb[W + 1];
    if (!(z00 < 0.f && z01 < 0.f && z10 < 0.f && z11 < 0.f)) return false;
    // 5. depth test against the nearest pixel centre
    const float zt = tv >= 0.5f ? (tu >= 0.5f ? z11 : z10) : (tu >= 0.5f ? z01 : z00);
    const float depth = -pz;
    const float bias = slack * depth * 2.0f / fminf(fx * Wf, fy * Hf) * sqrtf(fmaxf(1.0f - c * c, 0.f)) / c + 1e-4f * depth;
    if (!(pz >= zt - bias)) return false;
    t.c = c; t.tu = tu; t.tv = tv; t.off = off;
    return true;
}

// step 6's sample: t points at the top-left tap of one channel's plane
__device__ __forceinline__ float view_bilinear(const float *t, int W, float tu, float tv) {
    const float top = t[0] + tu * (t[1] - t[0]), bot = t[W] + tu * (t[W + 1] - t[W]);
    return top + tv * (bot - top);
}

}  // namespace lnerf
