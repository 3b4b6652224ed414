// Texture baking over a mesh's UV atlas: NeRFRenderer.bake_texture's kernels.  Contract: include/lnerf_hip.h,
// lnerf_uv_raster / lnerf_uv_dilate; numpy restatement: tests/uv_reference.py.
//
// lnerf_uv_raster, stage by stage (every pass linear in its work, no cross-workgroup waiting):
//   ITEMS  k_uv_setup  one lane per face: pixel-space corners, area, candidate box; items = box area; an in-block
//                      exclusive prefix of the items (int64) and per-block item / bad-index totals
//          scan_top    (scan.h) ONE workgroup: exclusive prefix of the block totals (in place) -> counts[0] items,
//                      [1] bad faces
//   COVER  k_uv_cover  one lane per (face, box texel) item, so one big UV triangle does not serialise on one lane:
//                      the item's face by binary search over the item prefix, the edge test, atomicMax of the face
//                      index into texel_face (the largest covering index wins, whatever the order)
//          k_uv_count  one lane per texel: covered texels per block of UV_THREADS texels
//          scan_top    exclusive prefix of those -> counts[2] = P
//   EMIT   k_uv_emit   one lane per texel: rank among the block's covered texels (ballot / mbcnt + wave totals in LDS),
//                      texel_idx and the surface point at block prefix + rank (ascending linear order)
// lnerf_uv_dilate: one launch per gutter round (k_uv_dilate), ping-ponging between the caller's two buffers.
#include "common.h"
#include "scan.h"
#include "uv_shared.h"

namespace lnerf {

__device__ __forceinline__ bool uv_indices_ok(const UvMesh &m, int f) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = m.faces[(int64_t)f * 3 + k], t = m.ft[(int64_t)f * 3 + k];
        ok = ok && v >= 0 && v < m.n_verts && t >= 0 && t < m.n_vt;
    }
    return ok;
}

__global__ void __launch_bounds__(UV_THREADS)
k_uv_setup(UvMesh m, int64_t *__restrict__ face_off, int64_t *__restrict__ blk_items, int64_t *__restrict__ blk_bad) {
    const int f = blockIdx.x * UV_THREADS + threadIdx.x;
    long long items = 0, bad = 0;
    if (f < m.n_faces) {
        if (uv_indices_ok(m, f)) {
            UvTri t;
            uv_tri(m, f, t);
            items = (long long)t.w * t.h;
        } else {
            bad = 1;
        }
    }
    const long long n[2] = {items, bad};
    long long excl[2], total[2];
    block_exclusive_scan<UV_THREADS>(n, excl, total);
    if (f < m.n_faces) face_off[f] = excl[0];
    if (threadIdx.x == 0) {
        blk_items[blockIdx.x] = total[0];
        blk_bad[blockIdx.x] = total[1];
    }
}

// items [base, base + n) of the stage's item list; lanes past the device total (counts[0]) do nothing
__global__ void __launch_bounds__(UV_THREADS)
k_uv_cover(UvMesh m, const int64_t *__restrict__ face_off, const int64_t *__restrict__ blk_items, int64_t nb,
           const int64_t *__restrict__ counts, int64_t base, int64_t n, int32_t *__restrict__ texel_face) {
    const int64_t t = base + (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    if (t >= base + n || t >= counts[0]) return;
    int r;
    const int f = uv_item_face(face_off, blk_items, nb, m.n_faces, t, r);
    UvTri tri;
    uv_tri(m, f, tri);
    const int di = r / tri.w;
    const int i = tri.i0 + di, j = tri.j0 + (r - di * tri.w);
    float e[3];
    if (uv_cover(tri, i, j, e)) atomicMax(&texel_face[(int64_t)i * m.R + j], f);
}

__global__ void __launch_bounds__(UV_THREADS)
k_uv_count(const int32_t *__restrict__ texel_face, int64_t n, int64_t *__restrict__ blk_texels) {
    __shared__ int s_n[UV_WAVES];
    const int64_t p = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    const bool c = p < n && texel_face[p] >= 0;
    const int cnt = (int)__popcll(__ballot(c));
    if (lane_id() == 0) s_n[threadIdx.x / LNERF_WAVE] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < UV_WAVES; ++k) s += s_n[k];
        blk_texels[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(UV_THREADS)
k_uv_emit(UvMesh m, const int32_t *__restrict__ texel_face, const int64_t *__restrict__ blk_texels,
          int32_t *__restrict__ texel_idx, float *__restrict__ pos, int64_t max_texels) {
    __shared__ int s_n[UV_WAVES];
    const int64_t n = (int64_t)m.R * m.R;
    const int64_t p = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    const int f = p < n ? texel_face[p] : -1;
    const unsigned long long mask = __ballot(f >= 0);
    const int w = threadIdx.x / LNERF_WAVE;
    if (lane_id() == 0) s_n[w] = (int)__popcll(mask);
    __syncthreads();
    if (f < 0) return;
    int before = 0;
#pragma unroll
    for (int k = 0; k < UV_WAVES; ++k)
        if (k < w) before += s_n[k];
    const int64_t q = blk_texels[blockIdx.x] + before + mbcnt(mask);
    if (q >= max_texels) return;
    const int i = (int)(p / m.R), j = (int)(p - (int64_t)i * m.R);
    UvTri tri;
    uv_tri(m, f, tri);
    float e[3];
    uv_cover(tri, i, j, e);
    const float b0 = e[0] / tri.area, b1 = e[1] / tri.area, b2 = e[2] / tri.area;
    const int64_t v0 = m.faces[(int64_t)f * 3], v1 = m.faces[(int64_t)f * 3 + 1], v2 = m.faces[(int64_t)f * 3 + 2];
    texel_idx[q] = (int32_t)p;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        pos[q * 3 + a] = b0 * m.verts[v0 * 3 + a] + b1 * m.verts[v1 * 3 + a] + b2 * m.verts[v2 * 3 + a];
}

// one gutter round: covered / filled texels are copied, an empty one takes the mean of its non-empty 8-neighbours
__global__ void __launch_bounds__(UV_THREADS)
k_uv_dilate(const float *__restrict__ src, const uint8_t *__restrict__ msrc, float *__restrict__ dst,
            uint8_t *__restrict__ mdst, int C, int R) {
    const int64_t n = (int64_t)R * R;
    const int64_t p = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint8_t mk = msrc[p];
    if (mk != 0) {
        for (int c = 0; c < C; ++c) dst[c * n + p] = src[c * n + p];
        mdst[p] = mk;
        return;
    }
    const int i = (int)(p / R), j = (int)(p - (int64_t)i * R);
    uint32_t nb = 0;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        if (k == 4) continue;
        const int ii = i + k / 3 - 1, jj = j + k % 3 - 1;
        if (ii >= 0 && ii < R && jj >= 0 && jj < R && msrc[(int64_t)ii * R + jj] != 0) {
            nb |= 1u << k;
            ++cnt;
        }
    }
    for (int c = 0; c < C; ++c) {
        const float *s = src + c * n;
        float v = s[p];
        if (cnt > 0) {
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if ((nb >> k) & 1u) sum += s[(int64_t)(i + k / 3 - 1) * R + (j + k % 3 - 1)];
            v = sum / (float)cnt;
        }
        dst[c * n + p] = v;
    }
    mdst[p] = cnt > 0 ? 1 : 0;
}

struct UvLayout {
    int64_t nbF, nbT;
    size_t face_off, blk_items, blk_bad, blk_texels, bytes;
};

static UvLayout uv_layout(int n_faces, int R) {
    UvLayout L;
    Carve c;
    L.nbF = div_up(n_faces, UV_THREADS);
    L.nbT = div_up((int64_t)R * R, UV_THREADS);
    L.face_off = c.take((size_t)n_faces * 8);
    L.blk_items = c.take((size_t)L.nbF * 8);
    L.blk_bad = c.take((size_t)L.nbF * 8);
    L.blk_texels = c.take((size_t)L.nbT * 8);
    L.bytes = c.o;
    return L;
}

}  // namespace lnerf

using namespace lnerf;

extern "C" {

size_t lnerf_uv_raster_scratch_bytes(int n_faces, int R) {
    if (n_faces < 0 || R < 1 || R > LNERF_UV_MAX_RES) return 0;
    return uv_layout(n_faces, R).bytes;
}

int lnerf_uv_raster(const float *verts, int n_verts, const int32_t *faces, const float *vt, int n_vt,
                    const int32_t *ft, int n_faces, int R, int stages, int64_t n_items, void *scratch,
                    size_t scratch_bytes, int32_t *texel_face, int32_t *texel_idx, float *pos, int64_t max_texels,
                    int64_t *counts_dev, lnerf_stream_t stream) {
    LNERF_REQUIRE(R >= 1 && R <= LNERF_UV_MAX_RES, "uv_raster: resolution %d outside [1, %d]", R, LNERF_UV_MAX_RES);
    LNERF_REQUIRE(n_faces >= 0 && n_verts >= 0 && n_vt >= 0, "uv_raster: negative count");
    LNERF_REQUIRE((stages & ~(LNERF_UV_ITEMS | LNERF_UV_COVER | LNERF_UV_EMIT)) == 0 && stages != 0,
                  "uv_raster: bad stage bits 0x%x", stages);
    LNERF_REQUIRE(scratch && counts_dev, "uv_raster: null pointer");
    LNERF_REQUIRE(n_faces == 0 || (verts && faces && vt && ft), "uv_raster: null mesh pointer");
    LNERF_REQUIRE(!(stages & (LNERF_UV_COVER | LNERF_UV_EMIT)) || texel_face, "uv_raster: null texel_face");
    LNERF_REQUIRE(!(stages & LNERF_UV_COVER) || n_items >= 0, "uv_raster: negative item count");
    LNERF_REQUIRE(!(stages & LNERF_UV_EMIT) || (max_texels >= 0 && (max_texels == 0 || (texel_idx && pos))),
                  "uv_raster: null output buffer with a non-zero capacity");
    const UvLayout L = uv_layout(n_faces, R);
    LNERF_REQUIRE(scratch_bytes >= L.bytes, "uv_raster: scratch of %zu bytes, need %zu", scratch_bytes, L.bytes);
    LNERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "uv_raster: scratch must be 16-byte aligned");
    UvMesh m;
    m.verts = verts; m.faces = faces; m.vt = vt; m.ft = ft;
    m.n_verts = n_verts; m.n_vt = n_vt; m.n_faces = n_faces; m.R = R;
    m.Rf = (float)R;
    int64_t *face_off = at<int64_t>(scratch, L.face_off), *blk_items = at<int64_t>(scratch, L.blk_items);
    int64_t *blk_bad = at<int64_t>(scratch, L.blk_bad), *blk_texels = at<int64_t>(scratch, L.blk_texels);
    const int64_t n_texels = (int64_t)R * R;
    hipStream_t s = as_stream(stream);
    if (stages & LNERF_UV_ITEMS) {
        if (n_faces > 0) {
            LNERF_LAUNCH(k_uv_setup, n_faces, UV_THREADS, s, m, face_off, blk_items, blk_bad);
            LNERF_CHECK_LAUNCH("uv_raster(setup)");
        }
        scan_top(blk_items, blk_bad, L.nbF, counts_dev, counts_dev + 1, s);
        LNERF_CHECK_LAUNCH("uv_raster(scan items)");
    }
    if (stages & LNERF_UV_COVER) {
        if (!hip_ok(hipMemsetAsync(texel_face, 0xff, (size_t)n_texels * 4, s), "uv_raster: clearing texel_face"))
            return LNERF_ERR_HIP;
        for (int64_t base = 0; base < n_items; base += UV_ITEMS_PER_LAUNCH) {
            const int64_t n = min(n_items - base, UV_ITEMS_PER_LAUNCH);
            LNERF_LAUNCH(k_uv_cover, n, UV_THREADS, s, m, face_off, blk_items, L.nbF, counts_dev, base, n, texel_face);
            LNERF_CHECK_LAUNCH("uv_raster(cover)");
        }
        LNERF_LAUNCH(k_uv_count, n_texels, UV_THREADS, s, texel_face, n_texels, blk_texels);
        LNERF_CHECK_LAUNCH("uv_raster(count)");
        scan_top(blk_texels, nullptr, L.nbT, counts_dev + 2, nullptr, s);
        LNERF_CHECK_LAUNCH("uv_raster(scan texels)");
    }
    if ((stages & LNERF_UV_EMIT) && max_texels > 0) {
        LNERF_LAUNCH(k_uv_emit, n_texels, UV_THREADS, s, m, texel_face, blk_texels, texel_idx, pos, max_texels);
        LNERF_CHECK_LAUNCH("uv_raster(emit)");
    }
    return LNERF_OK;
}

int lnerf_uv_dilate(float *texture, uint8_t *mask, int C, int R, int passes, float *tmp_texture, uint8_t *tmp_mask,
                    lnerf_stream_t stream) {
    LNERF_REQUIRE(R >= 1 && R <= LNERF_UV_MAX_RES, "uv_dilate: resolution %d outside [1, %d]", R, LNERF_UV_MAX_RES);
    LNERF_REQUIRE(C >= 1 && passes >= 0, "uv_dilate: C = %d, passes = %d", C, passes);
    LNERF_REQUIRE(texture && mask && (passes == 0 || (tmp_texture && tmp_mask)), "uv_dilate: null pointer");
    const int64_t n = (int64_t)R * R;
    hipStream_t s = as_stream(stream);
    float *a = texture, *b = tmp_texture;
    uint8_t *ma = mask, *mb = tmp_mask;
    for (int r = 0; r < passes; ++r) {
        LNERF_LAUNCH(k_uv_dilate, n, UV_THREADS, s, a, ma, b, mb, C, R);
        LNERF_CHECK_LAUNCH("uv_dilate");
        float *t = a; a = b; b = t;
        uint8_t *mt = ma; ma = mb; mb = mt;
    }
    if (a != texture) {
        if (!hip_ok(hipMemcpyAsync(texture, a, (size_t)n * C * 4, hipMemcpyDeviceToDevice, s), "uv_dilate: copy-back") ||
            !hip_ok(hipMemcpyAsync(mask, ma, (size_t)n, hipMemcpyDeviceToDevice, s), "uv_dilate: copy-back"))
            return LNERF_ERR_HIP;
    }
    return LNERF_OK;
}

}  // extern "C"
