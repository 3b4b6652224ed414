// Pixel-space triangles of a UV atlas and the (face, candidate texel) item list, shared by the texture bake (uvbake.hip)
// and the chart atlas's fold check (atlas.hip).  Contract: include/lnerf_hip.h, lnerf_uv_raster.
#pragma once
#include "common.h"

namespace lnerf {

constexpr int UV_THREADS = 256;
constexpr int UV_LOG2 = 8;
constexpr int UV_WAVES = UV_THREADS / LNERF_WAVE;
constexpr int64_t UV_ITEMS_PER_LAUNCH = int64_t(1) << 30;

struct UvMesh {
    const float *verts;
    const int32_t *faces;
    const float *vt;
    const int32_t *ft;
    int n_verts, n_vt, n_faces, R;
    float Rf;
};

// one face in pixel space: corners, area (= E_01 at corner 2), candidate box [j0, j0 + w) x [i0, i0 + h)
struct UvTri {
    float X[3], Y[3], area;
    int j0, i0, w, h;
};

// corners, area and box of face f (its ft indices must be valid); w = h = 0 when it covers nothing
__device__ __forceinline__ void uv_tri(const UvMesh &m, int f, UvTri &t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int q = m.ft[(int64_t)f * 3 + k];
        t.X[k] = m.vt[(int64_t)q * 2] * m.Rf;
        t.Y[k] = (1.0f - m.vt[(int64_t)q * 2 + 1]) * m.Rf;
    }
    t.area = (t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
    t.j0 = t.i0 = t.w = t.h = 0;
    if (!(fabsf(t.area) <= 3.402823466e38f) || t.area == 0.f) return;     // NaN, infinite or degenerate
    const float top = m.Rf - 1.0f;
    const float xl = floorf(fminf(fminf(t.X[0], t.X[1]), t.X[2])) - 1.0f;
    const float xh = floorf(fmaxf(fmaxf(t.X[0], t.X[1]), t.X[2])) + 1.0f;
    const float yl = floorf(fminf(fminf(t.Y[0], t.Y[1]), t.Y[2])) - 1.0f;
    const float yh = floorf(fmaxf(fmaxf(t.Y[0], t.Y[1]), t.Y[2])) + 1.0f;
    if (xh < 0.f || yh < 0.f || xl > top || yl > top) return;
    t.j0 = (int)fmaxf(xl, 0.f);
    t.i0 = (int)fmaxf(yl, 0.f);
    t.w = (int)fminf(xh, top) - t.j0 + 1;
    t.h = (int)fminf(yh, top) - t.i0 + 1;
}

// E_ab at the centre of texel (i, j): (X_b - X_a) * (p_y - Y_a) - (Y_b - Y_a) * (p_x - X_a)
__device__ __forceinline__ float uv_edge(const UvTri &t, int a, int b, float px, float py) {
    return (t.X[b] - t.X[a]) * (py - t.Y[a]) - (t.Y[b] - t.Y[a]) * (px - t.X[a]);
}

// edge values (E_12, E_20, E_01) at texel (i, j)
__device__ __forceinline__ void uv_edges(const UvTri &t, int i, int j, float e[3]) {
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    e[0] = uv_edge(t, 1, 2, px, py);
    e[1] = uv_edge(t, 2, 0, px, py);
    e[2] = uv_edge(t, 0, 1, px, py);
}

// the bake's coverage: true iff each edge value has the sign of the area or is 0
__device__ __forceinline__ bool uv_cover(const UvTri &t, int i, int j, float e[3]) {
    uv_edges(t, i, j, e);
    return t.area > 0.f ? (e[0] >= 0.f && e[1] >= 0.f && e[2] >= 0.f) : (e[0] <= 0.f && e[1] <= 0.f && e[2] <= 0.f);
}

// the fold check's coverage: true iff each edge value has the sign of the area and none is 0
__device__ __forceinline__ bool uv_cover_strict(const UvTri &t, int i, int j) {
    float e[3];
    uv_edges(t, i, j, e);
    return t.area > 0.f ? (e[0] > 0.f && e[1] > 0.f && e[2] > 0.f) : (e[0] < 0.f && e[1] < 0.f && e[2] < 0.f);
}

// Item t of the item list (face_off: exclusive prefix of the items inside each block of UV_THREADS faces, blk_items:
// exclusive prefix of the nb block totals): its face, by two binary searches, and its rank among that face's items.
__device__ __forceinline__ int uv_item_face(const int64_t *__restrict__ face_off, const int64_t *__restrict__ blk_items,
                                            int64_t nb, int n_faces, int64_t t, int &rank) {
    // the block: largest b with blk_items[b] <= t (an empty block shares its prefix with the next one)
    int64_t lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (blk_items[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int64_t local = t - blk_items[lo];
    int flo = (int)(lo << UV_LOG2), fhi = min(flo + UV_THREADS, n_faces) - 1;
    while (flo < fhi) {
        const int mid = (flo + fhi + 1) >> 1;
        if (face_off[mid] <= local) flo = mid; else fhi = mid - 1;
    }
    rank = (int)(local - face_off[flo]);               // < w * h <= R^2
    return flo;
}

}  // namespace lnerf
