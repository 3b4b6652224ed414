// The raster family's arithmetic, once: raster.hip (forward), rastergrad.hip (its transposes, the antialiasing), texmip.hip
// (the UV footprint) and view_shared.h (the view bake) call these, so a backward differentiates the rounding its forward made
// and a bake projects a point to where the rasteriser put it.  f32, no fused multiply-add but the projection's written ones.
#pragma once
#include "common.h"

namespace lnerf {

// ---- the camera record, wherever it lives (host array, device memory, an LDS tile, a Cam): rotation rows = the camera's
// x, y, z axes in world space, the eye, fx, fy = 1 / tan(fov/2) (/ ratio)
constexpr int CAM_FLOATS = 14, CAM_ROT = 0, CAM_POS = 9, CAM_FX = 12, CAM_FY = 13;
struct Cam { float rec[CAM_FLOATS]; };   // by value: a kernel argument, or a lane's copy
__host__ __device__ __forceinline__ Cam cam_read(const float *rec) {
    Cam c;
    for (int i = 0; i < CAM_FLOATS; ++i) c.rec[i] = rec[i];
    return c;
}
// camera-space z and NDC xy of the world point (wx, wy, wz): image = (x * fx, y * fy) / (z * -1)
struct CamPoint { float z, x, y; };
__device__ __forceinline__ CamPoint cam_project(const float *cam, float wx, float wy, float wz) {
    const float *rot = cam + CAM_ROT, *pos = cam + CAM_POS;
    const float x = wx - pos[0], y = wy - pos[1], z = wz - pos[2];
    const float cx = fmaf(rot[0], x, fmaf(rot[1], y, rot[2] * z));
    const float cy = fmaf(rot[3], x, fmaf(rot[4], y, rot[5] * z));
    const float cz = fmaf(rot[6], x, fmaf(rot[7], y, rot[8] * z));
    return {cz, cx * cam[CAM_FX] / (-cz), cy * cam[CAM_FY] / (-cz)};
}

// ---- NDC of the centre of pixel (row i, column j), its inverse (centres at integers), flat pixel -> (view, row, column)
struct Ndc { float x, y; };
struct Pixel { int b, i, j; };
__device__ __forceinline__ Ndc pixel_centre(int i, int j, int H, int W) {
    return {(2.0f * (float)j + 1.0f) / (float)W - 1.0f, 1.0f - (2.0f * (float)i + 1.0f) / (float)H};
}
__device__ __forceinline__ float ndc_to_col(float X, float Wf) { return ((X + 1.0f) * Wf - 1.0f) * 0.5f; }
__device__ __forceinline__ float ndc_to_row(float Y, float Hf) { return ((1.0f - Y) * Hf - 1.0f) * 0.5f; }
__device__ __forceinline__ Pixel pixel_of(int64_t p, int H, int W) {
    const int64_t hw = (int64_t)H * W;
    const int b = (int)(p / hw), rem = (int)(p - b * hw), i = rem / W;
    return {b, i, rem - i * W};
}

// ---- the weights of a face at (px, py), in two stages, so that a rasteriser pays for the second (three divisions and a
// reciprocal) only inside the face.  One: twice the signed area (0: a degenerate face, no weights), then its reciprocal and
// the screen-space weights.  Two: q_k = w_k / z_k, the depth z = (sum_k q_k)^-1 and the perspective-correct b_k = q_k z.
struct FaceW { float inv, w0, w1, w2; };
struct FaceP { float q0, q1, q2, z, b0, b1, b2; };
__device__ __forceinline__ float face_area(float x0, float y0, float x1, float y1, float x2, float y2) {
    return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
}
__device__ __forceinline__ FaceW face_weights(float area, float px, float py, float x0, float y0, float x1, float y1,
                                              float x2, float y2) {
    FaceW r;
    const float e0 = (x1 - px) * (y2 - py) - (x2 - px) * (y1 - py);  // weight of vertex 0
    const float e1 = (x2 - px) * (y0 - py) - (x0 - px) * (y2 - py);  // weight of vertex 1
    r.inv = 1.0f / area;
    r.w0 = e0 * r.inv; r.w1 = e1 * r.inv; r.w2 = 1.0f - r.w0 - r.w1;
    return r;
}
__device__ __forceinline__ FaceP face_perspective(const FaceW &w, float z0, float z1, float z2) {
    FaceP r;
    r.q0 = w.w0 / z0; r.q1 = w.w1 / z1; r.q2 = w.w2 / z2;
    r.z = 1.0f / (r.q0 + r.q1 + r.q2);
    r.b0 = r.q0 * r.z; r.b1 = r.q1 * r.z; r.b2 = r.q2 * r.z;
    return r;
}

// ---- the sizes the batched kernels share: views (a grid axis), image (int16 boxes); per-pixel kernels add P and F
static int check_view_dims(const char *who, int B, int H, int W) {
    LNERF_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (got %d)", who, B);
    LNERF_REQUIRE(H >= 1 && W >= 1 && H <= 32767 && W <= 32767, "%s: H and W must be in [1, 32767] (got %d, %d)", who, H, W);
    return LNERF_OK;
}
static int check_raster_dims(const char *who, int B, int H, int W, int F) {
    if (int e = check_view_dims(who, B, H, W)) return e;
    LNERF_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "%s: B * H * W must be below 2^31", who);
    LNERF_REQUIRE(F >= 1 && F <= LNERF_MESH_MAX_FACES, "%s: n_faces must be in [1, %d] (got %d)", who, LNERF_MESH_MAX_FACES, F);
    return LNERF_OK;
}

}  // namespace lnerf
